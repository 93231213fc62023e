// yk_engine.hip - batched self-play: Coach.executeEpisode (Coach.py:34-72) driving
// MCTS.getActionProb / MCTS.search (MCTS.py:28-164) for thousands of games in lock-step.
//
// Lock-step semantics.  Every game runs simulation k of move m at the same time:
//   k_select         one wavefront per game walks its own tree from the root (UCB argmax
//                    over the compact valid set, transitions with the game's own RNG
//                    stream) to the first unexpanded state, a terminal, or a dead node;
//   k_forward        one batched f32-MFMA forward over all pending leaves (yk_net.hip);
//   k_expand_backup  one wavefront per game: exp(log_softmax), mask, numpy-pairwise
//                    renormalise, insert the node, back the value up the path.
// Within a game the simulations stay strictly sequential, so each game reproduces the
// reference's recursive search exactly (no virtual loss); only different games overlap.
//
// Data layout (per game): open-addressing index of node ids keyed by the
// 64-byte packed state; 96-byte node records; one arena holding, per expanded node, its
// prior P over the compact valid set (f32) and a u16 edge slot per valid action; 16-byte
// edges {Q (f64 value + python-type tag), N}.  Node/edge pools are double-buffered; at a
// real round change the survivors (round >= the root's round - the only nodes a game can
// ever reach again, since round_no never decreases) are compacted into the other buffer.
#include <math.h>

#include <algorithm>
#include <vector>

#include "yk_api.h"
#include "yk_common.h"
#include "yk_engine_dev.h"
#include "yk_forced.h"
#include "yk_fpu.h"
#include "yk_utility.h"
#include "yk_net.h"
#include "yk_optarg.h"
#include "yk_temper.h"

#define YK_MAX_GROUPS 8

using namespace yk;

namespace {

// (the node / edge records, EngDev, the error bits and the tree lookups: yk_engine_dev.h)

// numpy float32 pairwise-sum plan for n = 3226 (loops_utils.h.src @TYPE@_pairwise_sum)
struct PwPlan {
    int nleaf, nop, root;
    uint16_t start[64], len[64];
    uint8_t a[64], b[64];
};
constexpr int pw_build(PwPlan& p, int start, int n) {
    if (n <= 128) {
        p.start[p.nleaf] = (uint16_t)start;
        p.len[p.nleaf] = (uint16_t)n;
        return p.nleaf++;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    const int l = pw_build(p, start, n2);
    const int r = pw_build(p, start + n2, n - n2);
    p.a[p.nop] = (uint8_t)l;
    p.b[p.nop] = (uint8_t)r;
    return 64 + p.nop++;
}
constexpr PwPlan make_plan() {
    PwPlan p{};
    p.root = pw_build(p, 0, ASIZE);
    return p;
}
static __constant__ PwPlan c_pw = make_plan();
static_assert(make_plan().nleaf <= 64 && make_plan().nop <= 64, "pairwise plan too large");
// The expand kernel evaluates the plan as a register butterfly: that is exact iff the tree is
// perfect over 32 in-order leaves, every leaf 8-aligned with 8 <= len <= 128.
constexpr bool plan_is_butterfly() {
    const PwPlan p = make_plan();
    if (p.nleaf != 32 || p.nop != 31) return false;
    int first[128] = {}, cnt[128] = {};
    for (int i = 0; i < p.nleaf; i++) {
        if (p.start[i] % 8 != 0 || p.len[i] < 8 || p.len[i] > 128) return false;
        if (i > 0 && p.start[i] != p.start[i - 1] + p.len[i - 1]) return false;
        first[i] = i;
        cnt[i] = 1;
    }
    for (int o = 0; o < p.nop; o++) {
        const int a = p.a[o], b = p.b[o];
        if (cnt[a] != cnt[b] || first[a] + cnt[a] != first[b] || first[a] % (2 * cnt[a]) != 0) return false;
        first[64 + o] = first[a];
        cnt[64 + o] = 2 * cnt[a];
    }
    return p.root == 64 + p.nop - 1 && cnt[p.root] == 32;
}
static_assert(plan_is_butterfly(), "numpy's pairwise tree for 3226 is no longer a perfect 32-leaf tree");
constexpr int pw_gmax() {
    const PwPlan p = make_plan();
    int g = 0;
    for (int i = 0; i < p.nleaf; i++) g = p.len[i] / 8 > g ? p.len[i] / 8 : g;
    return g;
}
constexpr int pw_tmax() {
    const PwPlan p = make_plan();
    int t = 0;
    for (int i = 0; i < p.nleaf; i++) t = p.len[i] % 8 > t ? p.len[i] % 8 : t;
    return t;
}
constexpr int PW_GMAX = pw_gmax();  // 8-element groups in the longest leaf
constexpr int pw_gmin() {
    const PwPlan p = make_plan();
    int g = PW_GMAX;
    for (int i = 0; i < p.nleaf; i++) g = p.len[i] / 8 < g ? p.len[i] / 8 : g;
    return g;
}
constexpr int PW_GMIN = pw_gmin();  // and in the shortest: groups below it need no test
constexpr int PW_TMAX = pw_tmax() > 0 ? pw_tmax() : 1;  // longest n % 8 tail
constexpr int pw_lmax() {
    const PwPlan p = make_plan();
    int l = 0;
    for (int i = 0; i < p.nleaf; i++) l = p.len[i] > l ? p.len[i] : l;
    return l;
}
// A 5-dice leaf's valid actions are NCOMB apart (one per unused category): no two share a leaf of the
// plan, so a leaf's partial sum is then that one prior (the expansion's sparse path)
static_assert(NCOMB > pw_lmax(), "two category starts could share a leaf of the pairwise plan");
static_assert(PF_WCAP % 8 == 0 && PF_WCAP >= 16 && GAMES_PER_BLOCK * PF_WCAP * 4 <= 40 * 1024,
              "the prior window: whole float4 pairs, a slot per category, 16 waves per CU");
// The staged P write of the general path: the tree's root splits the row where leaf 16
// starts, lanes 0-31 hold the left half and lanes 32-63 the right; either half fits the window whole
constexpr int PW_NLEAF = make_plan().nleaf;
constexpr int PW_SPLIT = make_plan().start[PW_NLEAF / 2];
static_assert(PW_SPLIT % 8 == 0 && PW_SPLIT <= PF_WCAP && ASIZE - PW_SPLIT <= PF_WCAP,
              "both halves of the pairwise tree fit the prior window, float4s aligned");
static_assert(PW_SPLIT > NBID && (PW_SPLIT - NBID) / NCOMB < NCAT, "the split lies inside a category's block");
constexpr int PW_SPLIT_CAT = (PW_SPLIT - NBID) / NCOMB, PW_SPLIT_COMB = (PW_SPLIT - NBID) % NCOMB;  // 5, 146
// The second piece starts at the first leaf from which the rest of the row fits the window, below the
// split: a 10-dice leaf's group of four compact entries that the split cuts (146 = 2 mod 4) stays whole
constexpr int pw_leaf2() {
    const PwPlan p = make_plan();
    int i = 0;
    while (ASIZE - p.start[i] > PF_WCAP) i++;
    return i;
}
constexpr int PW_LEAF2 = pw_leaf2(), PW_BASE2 = make_plan().start[PW_LEAF2];
static_assert(PW_LEAF2 <= PW_NLEAF / 2 && PW_BASE2 % 8 == 0 && PW_BASE2 <= PW_SPLIT - (PW_SPLIT_COMB & 3),
              "the second piece holds the right half and the group the split cuts");

// getValidMoves of player 1 as wave-uniform scalars (the same test as action_valid)
struct ValidQ {
    int mode;       // 1: bid phase (a < 202), 0: score phase, -1: nothing valid
    int n;          // carry length
    uint32_t used;  // used categories
    __device__ __forceinline__ bool operator()(int a) const {
        if (mode == 1) return a < NBID;
        if (mode != 0 || a < NBID) return false;
        const int base = a - NBID, cat = base / NCOMB, ci = base - cat * NCOMB;
        if ((used >> cat) & 1u) return false;
        // the two carry sizes of real play need no table: 10 dice -> every combo, 5 -> combo 0
        if (n >= 10) return true;
        if (n == 5) return ci == 0;
        return c_tab.comb_max[ci] < n;
    }
};
__device__ __forceinline__ ValidQ valid_q(const YkS& s) {
    ValidQ q;
    const int round = s_round(s), phase = s_phase(s);
    const uint64_t wa = s_pw(s, 0, 0);
    q.n = __builtin_amdgcn_readfirstlane(wa_n(wa));
    q.used = __builtin_amdgcn_readfirstlane((uint32_t)wa_used(wa));
    q.mode = __builtin_amdgcn_readfirstlane((phase == 0 && round != 13) ? 1 : (phase == 1 && q.n >= 5) ? 0 : -1);
    return q;
}


// orders this wave's LDS / global accesses across lanes (waves of a block diverge, so no
// __syncthreads in per-game code)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, xlane<32>(v));
    v = fmaxf(v, xlane<16>(v));
    v = fmaxf(v, xlane<8>(v));
    v = fmaxf(v, xlane<4>(v));
    v = fmaxf(v, xlane<2>(v));
    return fmaxf(v, xlane<1>(v));
}
__device__ __forceinline__ float softmax_p(float x, float m, float lse) { return exp_acc(x - m - lse); }  // yk_common.h
__device__ __forceinline__ float wave_sumf(float v) {  // __shfl_xor's butterfly, bit for bit
    v += xlane<32>(v);
    v += xlane<16>(v);
    v += xlane<8>(v);
    v += xlane<4>(v);
    v += xlane<2>(v);
    return v + xlane<1>(v);
}
__device__ __forceinline__ int wave_min_i(int v) {
    v = min(v, xlane<32>(v));
    v = min(v, xlane<16>(v));
    v = min(v, xlane<8>(v));
    v = min(v, xlane<4>(v));
    v = min(v, xlane<2>(v));
    return min(v, xlane<1>(v));
}

// ------------------------------------------------------------------ python-typed arithmetic
// NEP 50 weak-scalar rules of numpy 2 (verified bitwise): any float32
// operand makes the result float32 (python ints/floats are cast to f32 first); python
// float with int -> float64; int / int -> float64 (true division).
struct PyV {
    double v;
    uint32_t t;
};
__device__ __forceinline__ PyV pv_update(PyV q, uint32_t n, PyV v) {  // (n*q + v) / (n+1)  MCTS.py:155-156
    PyV prod, sum, out;
    if (q.t == T_F32) prod = PyV{(double)((float)n * (float)q.v), T_F32};
    else prod = PyV{(double)n * q.v, q.t};
    if (prod.t == T_F32 || v.t == T_F32) sum = PyV{(double)((float)prod.v + (float)v.v), T_F32};
    else if (prod.t == T_F64 || v.t == T_F64) sum = PyV{prod.v + v.v, T_F64};
    else sum = PyV{prod.v + v.v, T_INT};
    if (sum.t == T_F32) out = PyV{(double)((float)sum.v / (float)(n + 1)), T_F32};
    else out = PyV{sum.v / (double)(n + 1), T_F64};
    return out;
}

// ------------------------------------------------------------------ kernels
__global__ void k_lut(float* sq, float* sqe) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= LUT_N) return;
    sq[i] = (float)sqrt((double)i);
    sqe[i] = (float)sqrt((double)i + 1e-8);
}

// reset every tree (MCTS() per episode, Coach.py:93) and, for self-play, start the games
__global__ void k_reset(EngDev d, int start_games, uint32_t env_base) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= d.E) return;
    for (int t = e; t < d.T; t += d.E) {  // the game's tree(s)
        d.node_count[t] = d.node_count[d.T + t] = 0;
        d.edge_count[t] = d.edge_count[d.T + t] = 0;
        d.arena_top[t] = 0;
        d.gen[t] = 0;
        d.cur_round[t] = 0;
        d.root_c[2 * t] = make_uint4(0, 0, 0, 0);
        d.root_c[2 * t + 1] = make_uint4(0, 0, RV_OFF, 0);
    }
#pragma unroll
    for (int k = 0; k < GST; k++) d.gstats[(long)e * GST + k] = 0;
    if (!start_games) return;
    d.env_id[e] = env_base + (uint32_t)e;
    Stream rs{d.seed, d.env_id[e], 0};
    YkS s;
#pragma unroll
    for (int k = 0; k < 8; k++) s.w[k] = 0;
    s.w[0] = 1ull | NO_BIDS;  // getInitBoard  YachtGame.py:232-237
    new_round_rolls(s, rs);
    st_state(d.board + e, s);
    d.cur[e] = 1;
    d.ctr[e] = rs.ctr;
    d.done[e] = 0;
    d.nmoves[e] = 0;
    d.rec_voff[(long)e * (d.M + 1)] = 0;
}

// Per move: root = canonical(board, cur)  (Coach.py:57); on a real round change compact the
// game's tree into the other buffer, keeping nodes whose round >= the root's.  One wave per game.
__global__ __launch_bounds__(256) void k_move_begin(EngDev d, int move, int external_root) {
    const int lane = threadIdx.x & 63;
    const int e = d.e_lo + blockIdx.x * GAMES_PER_BLOCK + (threadIdx.x >> 6);
    if (e >= d.e_hi) return;
    const int t = tree_of(d, e);
    if (lane == 0) {
        d.root_c[2 * t] = make_uint4(0, 0, 0, 0);  // ids move at a compaction: look the root up afresh
        d.root_c[2 * t + 1] = make_uint4(0, 0, RV_OFF, 0);  // the sorted root: rebuilt after the first expansion
    }
    if (!external_root) {
        if (d.done[e]) return;
        const YkS b = ld_state(d.board + e);
        const YkS r = canonical(b, d.cur[e]);
        const bool idle = d.arena && (d.cur[e] == d.seat[e] ? d.arena_agent : d.arena_opp) != YK_PLAYER_MCTS;
        if (lane == 0) {
            st_state(d.root + e, r);
            d.rec_ctr[((long)e * d.M + move) * 2] = d.ctr[e];
            d.idle[e] = idle ? 1 : 0;
        }
        if (idle) return;  // Arena: the random / greedy players do not search (YachtPlayers.py:174-214)
    } else if (lane == 0) {
        d.idle[e] = 0;
    }
    const YkS r = ld_state(d.root + e);
    const int rr = s_round(r);
    const int cr = d.cur_round[t];
    if (rr == cr) return;
    if (rr < cr) {
        if (lane == 0) atomicOr(d.err, ERR_ROUND);
        return;
    }
    // ---- compaction g -> g ^ 1 (in-place for the arena: survivors only move down)
    const int g = d.gen[t], h = g ^ 1;
    uint32_t* hx = d.hidx[h] + (long)t * d.HCAP;
    for (int i = lane; i < d.HCAP; i += 64) hx[i] = 0;
    const NodeRec* src = d.nodes[g] + (long)t * d.NCAP;
    NodeRec* dst = d.nodes[h] + (long)t * d.NCAP;
    const Edge* esrc = d.edges[g] + (long)t * d.ECAP;
    Edge* edst = d.edges[h] + (long)t * d.ECAP;
    float* P = d.arenaP + (long)t * d.AE;
    uint16_t* S = d.arenaS + (long)t * d.AE;
    const uint32_t cnt = d.node_count[g * d.T + t];
    uint32_t nn = 0, ne = 0, top = 0;
    wave_sync();
    // 64 records' rounds at a time (one load per lane), then the survivors in id order: the
    // records of earlier rounds cost no serial round trip
    for (uint32_t b0 = 0; b0 < cnt; b0 += 64) {
    const uint32_t il = b0 + (uint32_t)lane;
    uint64_t live = __ballot(il < cnt && (int)(src[il < cnt ? il : 0].key[0] & 0xF) >= rr);
    while (live) {
        const uint32_t id = b0 + (uint32_t)__builtin_ctzll(live);
        live &= live - 1;
        NodeRec rec = src[id];
        const int V = (int)rec.nvalid, VP = pad4(V);
        const uint32_t so = rec.p_off;
        for (int j0 = 0; j0 < VP; j0 += 64) {
            const int j = j0 + lane;
            float p = 0.f;
            uint16_t sl = 0;
            if (j < VP) {
                p = P[so + j];
                sl = S[so + j];
            }
            const bool vis = j < V && sl != 0;
            const uint64_t bal = __ballot(vis);
            const uint32_t before = __popcll(bal & ((1ull << lane) - 1));
            uint16_t nsl = 0;
            if (vis) {
                Edge x = esrc[sl - 1];
                x.tag = edge_kind(x.tag);  // node ids change: the cached child is dropped
                edst[ne + before] = x;
                nsl = (uint16_t)(ne + before + 1);
            }
            ne += (uint32_t)__popcll(bal);
            if (j < VP) {
                P[top + j] = p;
                S[top + j] = nsl;
            }
        }
        rec.p_off = top;
        top += (uint32_t)VP;
        if (lane == 0) {
            dst[nn] = rec;
            insert_index(d, h, t, rec.hash, nn);
        }
        nn++;
    }
    }
    if (lane == 0) {
        d.node_count[h * d.T + t] = nn;
        d.edge_count[h * d.T + t] = ne;
        d.arena_top[t] = top;
        d.gen[t] = (uint8_t)h;
        d.cur_round[t] = (uint8_t)rr;
    }
}


// The root's UCB argmax (MCTS.py:117-135) without scanning its whole compact set: the root is the
// same node for all of a move's simulations, and between two of them only one of its edges changes.
// An unvisited edge's u = (c P) sqrt(Ns + 1e-8) is monotone in P, so the best unvisited edge is the
// first unvisited entry of the root's P order (k_root_sort), and entries of equal u - the band that
// follows it in that order - go to the lowest index (strict '>' in ascending action order).  The
// visited edges (the list the backups append to) are scanned as before.  Same f32 operations as the
// full scan, so the same winner, bit for bit.  Returns the winner's compact index (0x7FFFFFFF: none)
// and its edge tag (0: unvisited), or -1 when the order's nk stored entries end before the walk does
// (the caller then scans the whole set); `scanned` counts the entries read.
// FORCED (a full self-play move with forced playouts): a visited edge that forced_edge names
// has u = +inf - only the visited list changes, an unvisited edge is never forced - and `fpick` is set when
// such an edge is the winner.
// FPU (first-play urgency): the visited list's loop also adds the two integer sums of the parent
// estimate, the walk is the same (x = (c P) sqe is monotone in P, so the band logic holds), and the last
// comparison is yk_fpu.h's: the visited list's winner against fq + ub.  `fcnt` gets 1 (the rule decided: the
// root has both kinds of edge) | 2 (the unvisited candidate won).
template <bool FORCED, bool FPU>
__device__ __forceinline__ int root_scan(const EngDev& d, int t, int lane, uint32_t nv, const float* P,
                                         const uint16_t* S, const Edge* edges, int V, int nk, int ws, float sq,
                                         float sqe, uint32_t& wtag, uint64_t& scanned, uint64_t& gathered,
                                         uint32_t Ns, double fk, int& fpick, double fr, int& fcnt) {
    const uint16_t* oj = d.ro_j + (long)t * RO_K;
    const float* op = d.ro_p + (long)t * RO_K;
    const uint32_t* rv = d.rv + (long)t * RV_CAP;
    // the walk starts at ws (every entry before it is visited: a visit is never undone within a
    // move); its first piece is loaded beside the visited list
    int jj = ws + lane < nk ? (int)oj[ws + lane] : 0;
    float pp = ws + lane < nk ? op[ws + lane] : 0.f;
    float best = -INFINITY;
    int bj = 0x7FFFFFFF;
    uint32_t btag = 0;
    int64_t fw = 0;   // FPU: this lane's part of W and of Mi
    uint64_t fm = 0;
    for (uint32_t i = (uint32_t)lane; i < nv; i += 64) {
        const uint32_t w = rv[i];
        const int j = (int)(w & 0xFFFu);
        const float p = P[j];
        const Edge ev = edges[(w >> 12) - 1];
        float u = (float)ev.Q + ((d.c32 * p) * sq) / (float)(ev.N + 1);
        if (FORCED && forced_edge(ev.N, p, Ns, fk)) u = INFINITY;
        if (FPU) {
            fw += fpu_w_term(ev.N, ev.Q);
            fm += fpu_m_term(p);
        }
        if (u > best || (u == best && j < bj)) {
            best = u;
            bj = j;
            btag = ev.tag;
        }
    }
    float ub = -INFINITY;
    int uj = 0x7FFFFFFF;
    bool found = false, done = false;
    int walked = 0;  // entries of the order read
    int first = nk;   // the order's first unvisited entry: the next walk's start
    for (int k0 = ws; k0 < nk; k0 += 64) {
        const int k = k0 + lane;
        if (k0 != ws) {
            jj = k < nk ? (int)oj[k] : 0;
            pp = k < nk ? op[k] : 0.f;
        }
        walked = min(k0 + 64, nk) - ws;
        const bool in = k < nk;
        const bool unv = in && S[jj] == 0;
        const float u = (d.c32 * pp) * sqe;
        bool cand;
        if (!found) {
            const uint64_t bal = __ballot(unv);
            if (!bal) continue;  // every entry of this piece is visited
            const int f = __builtin_ctzll(bal);
            ub = lane_val(u, f);
            found = true;
            first = k0 + f;
            cand = unv && lane >= f && u == ub;
        } else {
            cand = unv && u == ub;
        }
        uj = min(uj, wave_min_i(cand ? jj : 0x7FFFFFFF));
        // u is non-increasing along the order: the band goes on into the next piece only if the
        // piece's last entry still has u == ub
        if (!(k0 + 64 < nk && lane_val(u, 63) == ub)) {
            done = k0 + 64 < nk || nk == V || lane_val(u, (nk - 1 - k0) & 63) != ub;
            break;
        }
    }
    if (lane == 0 && first != ws) d.root_c[2 * t + 1].w = (uint32_t)first;
    if (!done && nk < V) {  // the stored order ended first: no unvisited entry among the top nk, or
        scanned += (uint64_t)nv + (uint64_t)walked;  // a band of equal u that may go on past them
        gathered += (uint64_t)nv;                     // (one edge per visited-list entry)
        return -1;
    }
    if (FPU) {  // the visited list's winner first, then yk_fpu.h's comparison (every lane holds every term)
        const int mine = bj;
        wave_argmax_step(best, bj);
        const uint64_t own = __ballot(mine == bj);
        wtag = own ? __builtin_amdgcn_readlane(btag, (int)__builtin_ctzll(own)) : 0u;
        const bool vis = bj != 0x7FFFFFFF;
        if (found && vis) {
            const float fq = fpu_value((int64_t)fpu_wave_sum((uint64_t)fw), fpu_wave_sum(fm), Ns, fr);
            fcnt = 1;
            if (fpu_unvisited_wins(fq, ub, uj, best, bj)) {
                fcnt = 3;
                best = ub;  // (finite: not a forced pick)
                bj = uj;
                wtag = 0u;
            }
        } else if (found) {
            best = ub;
            bj = uj;
            wtag = 0u;
        }
        if (FORCED) fpick = best == INFINITY;
        scanned += (uint64_t)nv + (uint64_t)walked;
        gathered += (uint64_t)nv;
        return bj;
    }
    if (lane == 0 && found && (ub > best || (ub == best && uj < bj))) {
        best = ub;
        bj = uj;
        btag = 0;
    }
    const int mine = bj;
    wave_argmax_step(best, bj);
    if (FORCED) fpick = best == INFINITY;  // (no other u is +inf: Q, P and the square roots are finite)
    const uint64_t own = __ballot(mine == bj);  // the lane whose own candidate won holds its tag
    wtag = own ? __builtin_amdgcn_readlane(btag, (int)__builtin_ctzll(own)) : 0u;
    scanned += (uint64_t)nv + (uint64_t)walked;
    gathered += (uint64_t)nv;
    return bj;
}

// A game without a descent this simulation (finished, or an arena seat that does not search)
__device__ __forceinline__ void select_none(const EngDev& d, int e, int lane) {
    if (lane == 0) {
        d.leaf_flag[e] = 0;
        d.path_len[e] = 0;
        d.end_node[e] = 0;
    }
}

// One simulation's descent (MCTS.search, MCTS.py:56-152 up to the recursion) of a game that searches
// (not done, not idle: the caller's test) in its tree t, generation g.  The caller passes t and g:
// the fused kernel's expansion holds them already, and re-reading done / idle / tree_of / gen[t]
// would put two more dependent round trips on every simulation's chain.
// All 64 lanes of the game's wave call it together.
//
// FORCED: the forced playouts of DESIGN.md s6f at depth 0, on every path the root's pick can take - root_scan's
// visited list, and the full scan (a move's first simulation, root_scan's -1, a visited list that overflowed,
// YK_ROOT_SCAN=0).  The node summary needs no case of its own: it decides a node only at Ns = 0, where no
// edge is visited, and only visited edges are forced.  The default instantiation is the code it was.
//
// Invariant (no node is terminal): the key of every node record is a state with game_ended == 0.
// The one writer of a new record is the expansion of a leaf, and a descent flags a leaf only after
// that state's Es test below came out 0; k_move_begin's compaction copies records unchanged, and the
// external-root and dual-tree paths insert through the same expansion into the tree they search.
// game_ended is a function of the state alone.  So a level whose node is already known - the cached
// root (root_c: set after a lookup that followed the test) or a cached child (an edge tag: the backup
// caches only ids of records, the next level's node, the new leaf or a node without valid actions;
// after a terminal break end_id is 0 and nothing is cached) - needs no Es test and no lookup.
//
// FPU: first-play urgency (the arithmetic of yk_fpu.h) at every node with Ns > 0 that has both a
// visited and an unvisited edge, on every path: root_scan, and the full scan, which then keeps two running bests
// (the visited u, the unvisited x) and the two integer sums per lane.  A node at Ns = 0 (the summary's, or a
// full scan over unvisited edges only) and a node whose edges are all visited come out as before.
//
// UTIL: the score-margin utility (the arithmetic of yk_utility.h) at the one place a terminal value
// enters the search, the Es test below: the descent returns -u(s, 1) in place of -Es, still a Python float, and
// counts the return.  Whether the state is terminal stays Es != 0.  Nothing else of the descent reads it.
template <bool FORCED, bool FPU, bool UTIL>
__device__ __forceinline__ void select_game(const EngDev& d, int e, int lane, int t, int g, const uint32_t* env_ids,
                                            uint64_t* ctr_arr, const ForcedDev& fd, const FpuDev& fp, const UtilDev& ud) {
    // FORCED: 1 when the root's pick was a forced edge.  (Declared first: among the locals below it reorders two
    // phi nodes of the default instantiation, and the register allocation with them.)
    int fpick = 0;
    // FPU: root_scan's report (1: the rule decided | 2: the unvisited candidate won), then the descent's picks the
    // rule decided and those of them the unvisited candidate won.  (Declared here for the same reason: as a local
    // of the root's block, fcnt rotates four phi nodes of the default instantiation.)
    int fcnt = 0;
    int fpu_n = 0, fpu_u = 0;
    YkS s = ld_state(d.root + e);
    Stream rs{d.seed, env_ids[e], ctr_arr[e]};
    const NodeRec* nodes = d.nodes[g] + (long)t * d.NCAP;
    const Edge* edges = d.edges[g] + (long)t * d.ECAP;
    const float* Pbase = d.arenaP + (long)t * d.AE;
    const uint16_t* Sbase = d.arenaS + (long)t * d.AE;
    uint64_t* path = d.path + (long)e * MAXD;
    int depth = 0;
    uint64_t scanned = 0, gathered = 0;  // UCB entries read; their edges gathered (visited entries)
    int ngl = 0;                          // this lane's edge gathers in full scans
    int leaf = 0;
    uint32_t end_id = 0;   // id + 1 of a node the descent stops at
    PyV res{0.0, T_INT};
    // this level's node when it is known before any lookup (the cached root, a cached child): its id
    // and fields, fetched in one batch
    bool have = false;
    int nid = -1;
    NodeF f{};
    // the root's pick from its P order and visited list (root_scan), made before the walk, where
    // little else is live (inside the loop the second scan path would spill)
    bool pre = false;
    int pre_bj = 0x7FFFFFFF;
    uint32_t pre_tag = 0;
    {
        // the root is the same node for every simulation of a move: its id and the record's fixed
        // fields are kept after the first lookup (root_c, read once per descent), which saves the
        // hash, the index probe and the key's compare; Ns and first_j come from the record
        const uint4 rc = d.root_c[2 * t], rc1 = d.root_c[2 * t + 1];
        const uint32_t rid = uni(rc.x);
        if (rid != 0) {
            have = true;
            nid = (int)rid - 1;
            f = ld_node(nodes + nid);
            f.p_off = rc.y;
            f.nvalid = rc.z;
            f.vinfo = (uint64_t)rc1.x | ((uint64_t)rc1.y << 32);
            f = uniform(f);
        }
        if (rid != 0 && uni(rc1.z) != RV_OFF) {  // k_root_sort ran this move: root_c holds the root
            const float sq = (float)sqrt((double)f.Ns), sqe = (float)sqrt((double)f.Ns + 1e-8);
            pre_bj = __builtin_amdgcn_readfirstlane(root_scan<FORCED, FPU>(
                d, t, lane, rc1.z, Pbase + rc.y, Sbase + rc.y, edges, (int)rc.z, (int)rc.w, (int)rc1.w, sq, sqe, pre_tag,
                scanned, gathered, f.Ns, fd.k, fpick, fp.r_root, fcnt));
            pre_tag = __builtin_amdgcn_readfirstlane(pre_tag);
            pre = pre_bj != -1;
            if (FORCED) fpick = pre ? __builtin_amdgcn_readfirstlane(fpick) : 0;
            if (FPU && pre) {
                fcnt = __builtin_amdgcn_readfirstlane(fcnt);
                fpu_n += fcnt & 1;
                fpu_u += fcnt >> 1;
            }
        }
    }
    while (true) {
        if (!have) {
            const double es = game_ended(s, 1);  // Es (MCTS.py:78-82)
            if (es != 0.0) {
                if constexpr (UTIL) {  // (s is canonical: seen from player 1)
                    res = PyV{-score_utility(s, 1, es, ud), T_F64};
                    if (lane == 0) atomicAdd(ud.terminals + e, 1ull);
                } else {
                    res = PyV{-es, T_F64};
                }
                break;
            }
            const uint64_t hsh = index_hash(s);
            nid = __builtin_amdgcn_readfirstlane(lookup(d, g, t, s, hsh, f));
            f = uniform(f);
            if (nid < 0) {  // leaf: predict (MCTS.py:84-115)
                leaf = 1;
                if (lane == 0) {
                    st_state(d.leaf_state + e, s);
                    d.leaf_hash[e] = hsh;
                }
                break;
            }
            if (depth == 0 && lane == 0) {  // the move's root, for its later descents
                d.root_c[2 * t] = make_uint4((uint32_t)nid + 1, f.p_off, f.nvalid, 0);
                d.root_c[2 * t + 1] = make_uint4((uint32_t)f.vinfo, (uint32_t)(f.vinfo >> 32), RV_OFF, 0);
            }
        }
        const uint32_t p_off = f.p_off;
        const int V = (int)f.nvalid;
        const uint64_t vinfo = f.vinfo;
        if (V == 0) {  // no valid action: MCTS.py:141-147 returns 0 (python int)
            res = PyV{0.0, T_INT};
            end_id = (uint32_t)nid + 1;
            break;
        }
        // UCB argmax, MCTS.py:117-135: float32 arithmetic, strict '>' => lowest action wins
        const uint32_t Ns = f.Ns;
        // f32(sqrt(Ns)), f32(sqrt(Ns + 1e-8)) (MCTS.py:125-129 under NEP 50): f64 sqrt is correctly
        // rounded, so these are the bits numpy gets; computed here rather than read from a table,
        // which saves a dependent load per level (expand 53.35 -> 53.02 us, profiles/r03_expand_ab.log)
        const float sq = (float)sqrt((double)Ns);
        const float sqe = (float)sqrt((double)Ns + 1e-8);
        const float* P = Pbase + p_off;
        const uint16_t* S = Sbase + p_off;
        int bj_out;
        uint32_t wtag;
        if (depth == 0 && pre) {  // the root: picked above from its P order and visited list
            bj_out = pre_bj;
            wtag = pre_tag;
        } else {
            float best = -INFINITY;
            int bj = 0x7FFFFFFF;
            uint32_t btag = 0;  // the edge tag of the lane's best entry (0: unvisited)
            // FPU: `best` / `bj` / `btag` are the visited candidate's, these the unvisited one's and the sums
            float bestx = -INFINITY;
            int bjx = 0x7FFFFFFF;
            int64_t fw = 0;
            uint64_t fm = 0;
            // the node summary (an interior node, or a root in full-scan mode): at Ns = 0 no edge is
            // visited and every term is (c P) sqe0, so the pick is the one the expansion stored.  It
            // seeds every lane and leaves the scan nothing to read (a second exit path here spills).
            int Vs = V;  // entries the full scan reads
            if (d.node_summary && Ns == 0) {
                bj = (int)f.first_j;
                Vs = 0;
            }
            // software-pipelined scan: iteration it+1's P / slot loads fly while iteration it's
            // visited-edge gathers resolve
            float4 p4 = make_float4(0.f, 0.f, 0.f, 0.f);
            ushort4 s4 = make_ushort4(0, 0, 0, 0);
            if (lane * 4 < Vs) {
                p4 = *reinterpret_cast<const float4*>(P + lane * 4);
                s4 = *reinterpret_cast<const ushort4*>(S + lane * 4);
            }
            for (int j0 = lane * 4; j0 < Vs; j0 += 256) {
                const float pv[4] = {p4.x, p4.y, p4.z, p4.w};
                const uint16_t sv[4] = {s4.x, s4.y, s4.z, s4.w};
                Edge ev[4];
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (j0 + t < Vs && sv[t]) {
                        ev[t] = edges[sv[t] - 1];
                        ngl++;
                    }
                if (j0 + 256 < Vs) {
                    p4 = *reinterpret_cast<const float4*>(P + j0 + 256);
                    s4 = *reinterpret_cast<const ushort4*>(S + j0 + 256);
                }
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int j = j0 + t;
                    if (j < Vs) {
                        float u;
                        const float cp = d.c32 * pv[t];
                        if (sv[t]) {
                            u = (float)ev[t].Q + (cp * sq) / (float)(ev[t].N + 1);
                            if (FORCED && depth == 0 && forced_edge(ev[t].N, pv[t], Ns, fd.k)) u = INFINITY;
                        } else {
                            u = cp * sqe;
                        }
                        if (FPU) {
                            if (sv[t]) {
                                fw += fpu_w_term(ev[t].N, ev[t].Q);
                                fm += fpu_m_term(pv[t]);
                                if (u > best) {
                                    best = u;
                                    bj = j;
                                    btag = ev[t].tag;
                                }
                            } else if (u > bestx) {
                                bestx = u;
                                bjx = j;
                            }
                        } else if (u > best) {
                            best = u;
                            bj = j;
                            btag = sv[t] ? ev[t].tag : 0u;
                        }
                    }
                }
            }
            if (Vs) wave_argmax_step(best, bj);  // (a stored pick: every lane holds it)
            if (FPU && Vs) {
                wave_argmax_step(bestx, bjx);
                const bool vis = bj != 0x7FFFFFFF, unv = bjx != 0x7FFFFFFF;
                bool unv_won = unv;  // (no visited edge: the unvisited candidate, as without the rule)
                if (vis && unv) {    // (Ns > 0: a visited edge was backed up through this node)
                    const float fq = fpu_value((int64_t)fpu_wave_sum((uint64_t)fw), fpu_wave_sum(fm), Ns, depth == 0 ? fp.r_root : fp.r);
                    unv_won = fpu_unvisited_wins(fq, bestx, bjx, best, bj);
                    fpu_n++;
                    fpu_u += unv_won;
                }
                // the unvisited candidate as the wave's best on every lane: finite (not a forced pick), tag 0.
                // What follows is then the code of the default instantiation, statement for statement
                if (unv_won) {
                    best = bestx;
                    bj = bjx;
                    btag = 0u;
                }
            }
            if (FORCED && depth == 0) fpick = best == INFINITY;
            scanned += (uint64_t)Vs;
            bj_out = bj;
            // the winner's lane holds its tag: its own best is the wave's (lowest j among equals)
            wtag = __builtin_amdgcn_readlane(btag, __builtin_amdgcn_readfirstlane((bj & 255) >> 2));
        }
        const int bj = bj_out;
        int j = bj;
        if (j == 0x7FFFFFFF) j = 0;  // MCTS.py:138-143: first valid action
        if (depth >= MAXD) {
            if (lane == 0) atomicOr(d.err, ERR_DEPTH);
            res = PyV{0.0, T_INT};
            break;
        }
        const uint32_t child = uni(bj == 0x7FFFFFFF ? 0u : (wtag >> 2));  // id + 1, 0: not cached
        if (child) {  // a deterministic transition taken before: the child node is known
            if (lane == 0) path[depth] = ((uint64_t)(p_off + (uint32_t)j) << 32) | (uint32_t)nid | PATH_DET;
            depth++;
            // the whole record in one batch, the fields first; the key is the state step + canonical
            // would give, which the next level needs only if it has to step
            have = true;
            nid = (int)child - 1;
            f = uniform(ld_node(nodes + nid));
            s = ld_state(reinterpret_cast<const yk_state_t*>(nodes[nid].key));
            continue;
        }
        have = false;
        const VInfo vi = unpack_vinfo(vinfo, (uint32_t)V);
        const int a = compact_to_action(vi, j);
        int np = 1;
        const uint64_t ctr0 = rs.ctr;
        const int st = step_state<true>(s, 1, a, rs, np);  // MCTS.py:149 (all lanes: wave-parallel dice)
        const uint32_t det = rs.ctr == ctr0 ? PATH_DET : 0u;  // no dice drawn: the child is a function of (s, a)
        if (lane == 0) path[depth] = ((uint64_t)(p_off + (uint32_t)j) << 32) | (uint32_t)nid | det;
        depth++;
        if (st != YK_ST_OK) {
            if (lane == 0) atomicOr(d.err, ERR_STEP);
            res = PyV{0.0, T_INT};
            break;
        }
        s = canonical(s, np);  // MCTS.py:150
    }
    gathered += (uint64_t)xlane_sum(ngl);
    if (lane == 0) {
        d.leaf_flag[e] = (uint8_t)(leaf ? (t < d.E ? 1 : 2) : 0);  // which net predicts it (dual trees)
        d.path_len[e] = (uint8_t)depth;
        d.end_node[e] = end_id;
        d.res_v[e] = res.v;
        d.res_t[e] = res.t;
        ctr_arr[e] = rs.ctr;
        // no-return atomics: nothing at the end of the game's chain waits for a counter's round trip
        unsigned long long* gs = reinterpret_cast<unsigned long long*>(d.gstats + (long)e * GST);
        atomicAdd(gs + 1, (unsigned long long)scanned);
        atomicAdd(gs + 2, (unsigned long long)depth);
        atomicAdd(gs + 7, 1ull);
        if (FORCED) atomicAdd(gs + 12, (unsigned long long)fpick);
        if (FPU) {
            atomicAdd(gs + 14, (unsigned long long)fpu_u);
            atomicAdd(gs + 15, (unsigned long long)fpu_n);
        }
        atomicAdd(gs + 8, (unsigned long long)gathered);
    }
}

// FD, the optional arguments (yk_optarg.h): ForcedDev for the FORCED instantiations (the launches of a full
// self-play move with forced playouts), then FpuDev for the FPU ones, then UtilDev for the
// score-margin utility's; nothing for the default.
using DescentArgs = yk::Args<ForcedDev, FpuDev, UtilDev>;
template <class... FD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_select(EngDev d, const uint32_t* env_ids, uint64_t* ctr_arr, FD... fd) {
    static_assert(yk::args_in(DescentArgs{}, yk::Args<FD...>{}), "ForcedDev, then FpuDev, then UtilDev, no further argument");
    constexpr bool FORCED = yk::has_arg<ForcedDev, FD...>, FPU = yk::has_arg<FpuDev, FD...>, UTIL = yk::has_arg<UtilDev, FD...>;
    const int lane = threadIdx.x & 63;
    // the wave's game as a scalar: every per-game base address is then scalar arithmetic, which keeps
    // the descent's vector registers for its scan (no scratch; as a vector value: 20 bytes per lane)
    const int e = __builtin_amdgcn_readfirstlane(d.e_lo + blockIdx.x * GAMES_PER_BLOCK + (threadIdx.x >> 6));
    if (e >= d.e_hi) return;
    if (d.done[e] || d.idle[e]) {
        select_none(d, e, lane);
        return;
    }
    const int t = __builtin_amdgcn_readfirstlane(tree_of(d, e));
    const int g = __builtin_amdgcn_readfirstlane((int)d.gen[t]);
    select_game<FORCED, FPU, UTIL>(d, e, lane, t, g, env_ids, ctr_arr, yk::opt_arg(ForcedDev{0.0, 0.0}, fd...), yk::opt_arg(FpuDev{0.0, 0.0}, fd...),
                                       yk::opt_arg(UtilDev{1.0, 0.0, 1.0, nullptr}, fd...));
}

// Leaf expansion (MCTS.py:84-115) and backup (MCTS.py:154-164) of this simulation, then -
// when do_select - the next simulation's descent for the same game (one kernel boundary per
// simulation fewer).  One wave per game.
__device__ __forceinline__ void expand_backup_game(const EngDev& d, int e, int lane, int t, int g);
template <class... FD>  // (FD: as k_select)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(YK_EXPAND_WPE))) void k_expand_backup(
    EngDev d, int do_select, const uint32_t* env_ids, uint64_t* ctr_arr, FD... fd) {
    static_assert(yk::args_in(DescentArgs{}, yk::Args<FD...>{}), "ForcedDev, then FpuDev, then UtilDev, no further argument");
    constexpr bool FORCED = yk::has_arg<ForcedDev, FD...>, FPU = yk::has_arg<FpuDev, FD...>, UTIL = yk::has_arg<UtilDev, FD...>;
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane(d.e_lo + blockIdx.x * GAMES_PER_BLOCK + (threadIdx.x >> 6));  // (as k_select)
    if (e >= d.e_hi) return;
    if (d.done[e]) return;
    // the game's tree and generation, once for the expansion, the backup and the descent
    const int t = __builtin_amdgcn_readfirstlane(tree_of(d, e));
    const int g = __builtin_amdgcn_readfirstlane((int)d.gen[t]);
    const bool idle = d.idle[e] != 0;  // (loaded with them, not after the backup)
    expand_backup_game(d, e, lane, t, g);
    if (do_select) {
        if (idle) {
            select_none(d, e, lane);
            return;
        }
        wave_sync();  // this wave's backup writes (edges, slots, Ns) precede its descent's reads
        select_game<FORCED, FPU, UTIL>(d, e, lane, t, g, env_ids, ctr_arr, yk::opt_arg(ForcedDev{0.0, 0.0}, fd...), yk::opt_arg(FpuDev{0.0, 0.0}, fd...),
                                       yk::opt_arg(UtilDev{1.0, 0.0, 1.0, nullptr}, fd...));
    }
}

__device__ __forceinline__ void expand_backup_game(const EngDev& d, int e, int lane, int t, int g) {
    PyV res{d.res_v[e], d.res_t[e]};
    uint32_t end_id = 0;  // id + 1 of the node the path's last edge leads to, if any
    if (d.leaf_flag[e]) {
        const YkS s = ld_state(d.leaf_state + e);
        const uint64_t ihsh = d.leaf_hash[e];                  // the index's hash
        const uint64_t hsh = d.prior == 1 ? key_hash(s) : 0ull;  // the hash prior's (spec) hash
        const VInfo vi = valid_info(s, 1);
        const ValidQ valid = valid_q(s);
        const int V = vi.V;
        // ---- prior, Ps * valids (MCTS.py:88) and np.sum(Ps) (MCTS.py:89), in registers.
        // Lane pair (2k, 2k+1) owns leaf k of numpy's float32 pairwise tree for n = 3226 (32
        // in-order leaves, 8-aligned): lane 2k+h holds elements 8j + 4h .. 8j + 4h + 3 of the
        // leaf (numpy's accumulators r[4h .. 4h+3]) and, for h = 0, its n % 8 tail.
        const int leaf = lane >> 1, h = lane & 1;
        const int st = c_pw.start[leaf], nl = c_pw.len[leaf], G = nl >> 3, R = nl & 7;
        float4 q[PW_GMAX];
        float qt[PW_TMAX];
        float v, mx = 0.f, lse = 0.f;
        const int pidx = (int)d.gstats[(long)e * GST + 0];
        // record_predictions samples games without changing the path: the production prior
        // below is what gets recorded (after masking, i.e. exactly what np.sum / P see)
        const bool rec = d.rec_pred && (e % d.rec_stride) == 0 && pidx < d.max_exp;
        const long rslot = rec ? (long)(e / d.rec_stride) * d.max_exp + pidx : 0;
        bool masked = false;  // q / qt already hold Ps * valids
        // The compact-first prior of a leaf with a small valid set: each unnormalised
        // prior is computed once, in compact order, and staged in the wave's LDS window; the pairwise
        // sum's operands and the P write below read it back, so neither runs a validity test or an exp.
        //   window (1): the valid actions span at most PF_WCAP floats (every bid node, a score node
        //               whose unused categories lie close together); the window is laid out by action
        //               from wbase, zeros between the categories
        //   sparse (2): a 5-dice score node, one action per unused category; slot = the category
        // A scalar choice per wave.  The general path (0) is the dense pass over all 3226 actions.
        __shared__ __attribute__((aligned(16))) float s_win[GAMES_PER_BLOCK][PF_WCAP];
        float* win = s_win[threadIdx.x >> 6];  // (only this wave touches it: wave_sync orders it)
        int fast = 0, wbase = 0, wlen = 0;
        if (d.prior_fast && V > 0) {
            if (valid.mode == 0 && valid.n == 5) {
                fast = 2;
                wlen = 16;
            } else {
                const int a0 = __builtin_amdgcn_readfirstlane(compact_to_action(vi, 0));
                const int a1 = __builtin_amdgcn_readfirstlane(compact_to_action(vi, V - 1));
                wbase = a0 & ~7;  // (a float4 of the sum's layout lies wholly inside or outside)
                wlen = (a1 + 1 - wbase + 7) & ~7;
                fast = wlen <= PF_WCAP ? 1 : 0;
            }
        }
        // an action's slot in the window
        const auto wslot = [&](int a) { return fast == 2 ? (a - NBID) / NCOMB : a - wbase; };
        // 10 dice: every combination is valid and a category's block is NCOMB = 0 mod 4 entries, so the compact
        // entries j .. j + 3 (j = 0 mod 4) are one category's consecutive actions a .. a + 3 with a = 2 mod 4
        // (category starts are NBID + NCOMB c): two 8-byte halves of the 16-byte aligned logits row and of
        // the window, whose base is 0 mod 8
        static_assert(NBID % 4 == 2 && NCOMB % 4 == 0 && PI_LD % 4 == 0, "a group of four is two aligned 8-byte halves");
        const bool score10 = valid.mode == 0 && valid.n >= 10;
        // a general leaf's priors are then computed four compact entries per lane, into the window piece by piece
        // and from there into q / qt
        const bool gquad = d.prior_fast >= 3 && fast == 0 && score10 && V > 0;
        if (d.prior == 0) {
            // pi = exp(log_softmax(logits)) (NNet.py:193) at the valid actions only: the forward
            // supplies each row's (max, log sum exp), so the invalid logits are never read
            const float2 ml = d.mlse[e];
            mx = ml.x;
            lse = ml.y;
            if (d.fparts > 1) {  // merge the head parts' (max, sum exp), in part order
                float ms = ml.y;
                for (int p = 1; p < d.fparts; p++) {
                    const float2 q = d.mlse[(long)p * d.E + e];
                    const float mm = fmaxf(mx, q.x);
                    if (mm != -INFINITY) {
                        ms = ms * exp_acc(mx - mm) + q.y * exp_acc(q.x - mm);
                        mx = mm;
                    }
                }
                lse = logf(ms);
            }
            v = d.vpred[e];
        } else {
            v = hash_prior_v(hsh);
        }
        // The unnormalised priors of a 10-dice score node's compact entries [jlo, jhi) (both 0 mod 4) into the
        // window laid out by action from wb: lane l takes the entries 4l .. 4l + 3 of each 256 - one action
        // computation (compact_to_action's 10-dice form), two 8-byte loads of the row, four priors (the dense
        // pass's expressions on the same operands) and two 8-byte window writes; four iterations' loads in
        // flight per lane, no range test per entry.  Only valid actions' logits are read.
        const auto quad_priors = [&](int jlo, int jhi, int wb) {
            const float* __restrict__ xr = d.logits + (long)e * PI_LD;
            for (int j0 = jlo + 4 * lane; j0 < jhi; j0 += 1024) {
                int aa[4];
                float2 x01[4], x23[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int j = j0 + 256 * u, ci = j / NCOMB;
                    const bool in = j < jhi;
                    aa[u] = in ? NBID + NCOMB * (int)((vi.cats >> (4 * ci)) & 0xF) + (j - ci * NCOMB) : NBID;
                    x01[u] = (d.prior == 0 && in) ? *reinterpret_cast<const float2*>(xr + aa[u]) : make_float2(0.f, 0.f);
                    x23[u] = (d.prior == 0 && in) ? *reinterpret_cast<const float2*>(xr + aa[u] + 2) : make_float2(0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (j0 + 256 * u < jhi) {
                        float* w = win + (aa[u] - wb);
                        if (d.prior == 0) {
                            *reinterpret_cast<float2*>(w) = make_float2(softmax_p(x01[u].x, mx, lse), softmax_p(x01[u].y, mx, lse));
                            *reinterpret_cast<float2*>(w + 2) = make_float2(softmax_p(x23[u].x, mx, lse), softmax_p(x23[u].y, mx, lse));
                        } else {
                            *reinterpret_cast<float2*>(w) = make_float2(hash_prior_pi(hsh, aa[u]), hash_prior_pi(hsh, aa[u] + 1));
                            *reinterpret_cast<float2*>(w + 2) = make_float2(hash_prior_pi(hsh, aa[u] + 2), hash_prior_pi(hsh, aa[u] + 3));
                        }
                    }
            }
        };
        if (fast) {
            for (int i = 4 * lane; i < wlen; i += 256) *reinterpret_cast<float4*>(win + i) = make_float4(0.f, 0.f, 0.f, 0.f);
            wave_sync();
            const float* __restrict__ xr = d.logits + (long)e * PI_LD;
            for (int j0 = lane; j0 < V; j0 += 256) {  // four gathers in flight per lane
                float xa[4];
                int aa[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int j = j0 + 64 * u;
                    aa[u] = j < V ? compact_to_action(vi, j) : 0;
                    xa[u] = (d.prior == 0 && j < V) ? xr[aa[u]] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (j0 + 64 * u < V)
                        win[wslot(aa[u])] = d.prior == 0 ? softmax_p(xa[u], mx, lse) : hash_prior_pi(hsh, aa[u]);
            }
            wave_sync();
            // the sum's operands from the window: zeros outside it
            int soff = -8;               // sparse: where the leaf's one category start lies in it (none: -8)
            float4 sv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (fast == 2) {
                const int c = st <= NBID ? 0 : (st - NBID + NCOMB - 1) / NCOMB;
                const int o = NBID + NCOMB * c - st;
                if (c < NCAT && o < nl) {
                    const float pc = win[c];
                    soff = o;
                    sv = make_float4((o & 3) == 0 ? pc : 0.f, (o & 3) == 1 ? pc : 0.f, (o & 3) == 2 ? pc : 0.f,
                                     (o & 3) == 3 ? pc : 0.f);
                }
            }
#pragma unroll
            for (int j = 0; j < PW_GMAX; j++) {
                const int o = 8 * j + 4 * h;
                float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                if (fast == 1) {
                    const int i = st + o - wbase;
                    if (j < G && (unsigned)i < (unsigned)wlen) w = *reinterpret_cast<const float4*>(win + i);
                } else if (j < G && o == (soff & ~3)) {
                    w = sv;
                }
                q[j] = w;
            }
#pragma unroll
            for (int r = 0; r < PW_TMAX; r++) {
                const int o = 8 * G + r, i = st + o - wbase;
                float w = 0.f;
                if (h == 0 && r < R) {
                    if (fast == 1) {
                        if ((unsigned)i < (unsigned)wlen) w = win[i];
                    } else if (o == soff) {
                        w = win[wslot(st + o)];
                    }
                }
                qt[r] = w;
            }
            masked = true;
        } else if (gquad) {
            // A general leaf at 10 dice: q / qt compact-first, through the window in the two pieces of the staged P
            // write below - the actions below PW_SPLIT from window base 0 for lanes 0-31 (the left half of the
            // pairwise tree), then the actions from PW_SPLIT on from base PW_BASE2 for lanes 32-63.  Per piece:
            // zeros, the priors of the compact entries that fall in it, and each lane's leaf read back as the dense
            // pass lays it out - an exp per valid action where the dense pass evaluates 52 per lane.  The group
            // the split cuts (category PW_SPLIT_CAT's combinations 144 .. 147, PW_SPLIT_COMB = 2 mod 4 between
            // its 8-byte halves) is computed in both pieces: either window holds all four of its actions, and
            // no lane reads the two on the far side of the split.
            const uint32_t un = ~valid.used & ((1u << NCAT) - 1u);
            const int cut = (int)((un >> PW_SPLIT_CAT) & 1u);
            const int jL = NCOMB * __builtin_popcount(un & ((1u << PW_SPLIT_CAT) - 1u)) + (cut ? (PW_SPLIT_COMB & ~3) : 0);
            static_assert(PW_SPLIT + 2 <= PF_WCAP && ((ASIZE - PW_BASE2 + 3) & ~3) <= PF_WCAP && PW_SPLIT % 4 == 0,
                          "the cut group and the zero fill stay inside the window");
#pragma unroll
            for (int pc = 0; pc < 2; pc++) {
                const int wb = pc ? PW_BASE2 : 0, wn = pc ? ((ASIZE - PW_BASE2 + 3) & ~3) : PW_SPLIT;
                if (pc) wave_sync();  // the first piece's reads precede the second piece's zeros
                for (int i = 4 * lane; i < wn; i += 256) *reinterpret_cast<float4*>(win + i) = make_float4(0.f, 0.f, 0.f, 0.f);
                wave_sync();
                quad_priors(pc ? jL : 0, pc ? V : jL + 4 * cut, wb);
                wave_sync();
                if ((lane >> 5) == pc) {
                    const float* wl = win + (st - wb);
#pragma unroll
                    for (int j = 0; j < PW_GMAX; j++)
                        q[j] = (j < PW_GMIN || j < G) ? *reinterpret_cast<const float4*>(wl + 8 * j + 4 * h)
                                                      : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int r = 0; r < PW_TMAX; r++) qt[r] = (h == 0 && r < R) ? wl[8 * G + r] : 0.f;
                }
            }
            wave_sync();  // the reads precede the staged write's stores to the window
            masked = true;
        } else if (d.prior == 0) {
            const float* x = d.logits + (long)e * PI_LD + st;
            // score actions at 10 dice (most leaves): a group a .. a + 3 (a = 0 mod 4) holds at
            // most two categories, a's and a + 2's (category starts are 202 + 252 c = 2 mod 4)
#pragma unroll
            for (int j = 0; j < PW_GMAX; j++) {
                const int a = st + 8 * j + 4 * h;
                bool v0, v1, v2, v3;
                if (score10) {
                    const int b0 = a - NBID, b2 = a + 2 - NBID;
                    const bool lo = j < G && b0 >= 0 && !((valid.used >> ((unsigned)b0 / NCOMB)) & 1u);
                    const bool hi = j < G && b2 >= 0 && !((valid.used >> ((unsigned)b2 / NCOMB)) & 1u);
                    v0 = v1 = lo;
                    v2 = v3 = hi;
                } else {
                    v0 = j < G && valid(a);
                    v1 = j < G && valid(a + 1);
                    v2 = j < G && valid(a + 2);
                    v3 = j < G && valid(a + 3);
                }
                float4 x4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v0 || v1 || v2 || v3) x4 = *reinterpret_cast<const float4*>(x + 8 * j + 4 * h);
                q[j] = make_float4(v0 ? softmax_p(x4.x, mx, lse) : 0.f, v1 ? softmax_p(x4.y, mx, lse) : 0.f,
                                   v2 ? softmax_p(x4.z, mx, lse) : 0.f, v3 ? softmax_p(x4.w, mx, lse) : 0.f);
            }
#pragma unroll
            for (int r = 0; r < PW_TMAX; r++)
                qt[r] = (h == 0 && r < R && valid(st + 8 * G + r)) ? softmax_p(x[8 * G + r], mx, lse) : 0.f;
            masked = true;
        } else {
#pragma unroll
            for (int j = 0; j < PW_GMAX; j++) {
                const int a = st + 8 * j + 4 * h;
                q[j] = j < G ? make_float4(hash_prior_pi(hsh, a), hash_prior_pi(hsh, a + 1), hash_prior_pi(hsh, a + 2),
                                           hash_prior_pi(hsh, a + 3))
                             : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int r = 0; r < PW_TMAX; r++) qt[r] = (h == 0 && r < R) ? hash_prior_pi(hsh, st + 8 * G + r) : 0.f;
        }
        // mask with the valid moves
#pragma unroll
        for (int j = 0; j < PW_GMAX; j++) {
            const int a = st + 8 * j + 4 * h;
            if (j < G && !masked) {
                if (!valid(a)) q[j].x = 0.f;
                if (!valid(a + 1)) q[j].y = 0.f;
                if (!valid(a + 2)) q[j].z = 0.f;
                if (!valid(a + 3)) q[j].w = 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < PW_TMAX; r++)
            if (h == 0 && r < R && !masked && !valid(st + 8 * G + r)) qt[r] = 0.f;
        if (rec) {  // Ps * valids (MCTS.py:88) of this expansion, the leaf and v
            float* rpi = d.rec_pi + rslot * ASIZE;
#pragma unroll
            for (int j = 0; j < PW_GMAX; j++)
                if (j < G) *reinterpret_cast<float4*>(rpi + st + 8 * j + 4 * h) = q[j];
#pragma unroll
            for (int r = 0; r < PW_TMAX; r++)
                if (h == 0 && r < R) rpi[st + 8 * G + r] = qt[r];
            if (lane == 0) {
                d.rec_v[rslot] = v;
                st_state(d.rec_leaf + rslot, s);
            }
        }
        // numpy pairwise_sum on the leaf: r_k = a[k] + a[8 + k] + ..., then
        // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail one by one
        float4 racc = q[0];
#pragma unroll
        for (int j = 1; j < PW_GMAX; j++)
            if (j < G) {
                racc.x += q[j].x;
                racc.y += q[j].y;
                racc.z += q[j].z;
                racc.w += q[j].w;
            }
        const float half = (racc.x + racc.y) + (racc.z + racc.w);
        const float other = xlane<1>(half);
        float lsum = h == 0 ? half + other : other + half;
#pragma unroll
        for (int r = 0; r < PW_TMAX; r++)
            if (r < R) lsum += qt[r];  // h = 0 holds the tail
        lsum = __builtin_bit_cast(float, dpp_mov<0xA0>(__builtin_bit_cast(uint32_t, lsum)));  // quad_perm [0,0,2,2]: the even lane's
        // the perfect tree over the 32 leaves, left + right at every level
        float y = xlane<2>(lsum);
        lsum = (lane & 2) ? y + lsum : lsum + y;
        y = xlane<4>(lsum);
        lsum = (lane & 4) ? y + lsum : lsum + y;
        y = xlane<8>(lsum);
        lsum = (lane & 8) ? y + lsum : lsum + y;
        y = xlane<16>(lsum);
        lsum = (lane & 16) ? y + lsum : lsum + y;
        y = xlane<32>(lsum);
        lsum = (lane & 32) ? y + lsum : lsum + y;
        const float sum = lsum;
        // ---- allocate + write P over the compact valid set, zero edge slots
        const int VP = pad4(V);
        const uint32_t off = d.arena_top[t];
        const uint32_t nid = d.node_count[g * d.T + t];
        bool ok = true;
        if ((int64_t)off + VP > d.AE) {
            if (lane == 0) atomicOr(d.err, ERR_ARENA);
            ok = false;
        }
        if (nid >= (uint32_t)d.NCAP) {
            if (lane == 0) atomicOr(d.err, ERR_NODES);
            ok = false;
        }
        if (ok) {
            float* P = d.arenaP + (long)t * d.AE + off;
            uint16_t* S = d.arenaS + (long)t * d.AE + off;
            const float inv_fallback = V > 0 ? 1.0f / (float)V : 0.0f;
            // P over the compact valid set (ascending action): Ps / sum, or the uniform fallback
            // (MCTS.py:90-107).  Written in compact order (coalesced): each prior read back from the
            // window, or with YK_PRIOR_FAST=0 / 1 on the general path recomputed exactly as above from the
            // L2-resident logits row (or the hash).
            const float* __restrict__ xr = d.logits + (long)e * PI_LD;
            // the node summary: the pick of the node's first UCB scan (Ns = 0: every term is
            // u = (c p) sqe0, the scan's own operations and order), from the final p's
            const float sqe0 = (float)sqrt((double)0u + 1e-8);
            float fb = -INFINITY;
            int fj = 0x7FFFFFFF;
            // A general leaf's priors are all in q / qt, laid out by action: the window takes them in two
            // pieces of whole leaves of the pairwise tree (zeros included, so no zero-fill) - the left half
            // (lanes 0-31, actions below PW_SPLIT), then the leaves from PW_LEAF2 on (actions from
            // PW_BASE2) - and the loop reads the compact entries [0, jA), then [jA, VP), back from it: no
            // second gather, no second exp.
            const bool staged = d.prior_fast >= 2 && !fast && V > 0;
            // 10 dice: every combination valid, a category's block is NCOMB = 0 mod 4 entries, so the
            // compact entries j .. j + 3 (j = 0 mod 4) are one category's consecutive actions
            const bool quad = staged && score10;
            // valid actions below the split (the compact order ascends by action); at 10 dice rounded down to
            // a whole group of four - the second piece's window holds the cut group's actions below the split
            int jA = 0;
            if (staged) {
                if (quad) {  // whole categories of NCOMB, then the cut one's head, down to a whole group
                    const uint32_t un = ~valid.used & ((1u << NCAT) - 1u);
                    jA = NCOMB * __builtin_popcount(un & ((1u << PW_SPLIT_CAT) - 1u)) +
                         (((un >> PW_SPLIT_CAT) & 1u) ? (PW_SPLIT_COMB & ~3) : 0);
                } else {
                    int lo = 0, hi = V;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (compact_to_action(vi, mid) < PW_SPLIT) lo = mid + 1;
                        else hi = mid;
                    }
                    jA = __builtin_amdgcn_readfirstlane(lo);
                }
            }
            const int nhalf = staged ? 2 : 1;
            for (int hf = 0; hf < nhalf; hf++) {
            const int jlo = hf ? jA : 0, jhi = (staged && !hf) ? jA : VP;
            if (staged) {
                wbase = hf ? PW_BASE2 : 0;
                if (hf) wave_sync();  // the first piece's reads precede the second piece's writes
                if (hf ? leaf >= PW_LEAF2 : leaf < PW_NLEAF / 2) {
                    float* wl = win + (st - wbase);
#pragma unroll
                    for (int j = 0; j < PW_GMAX; j++)
                        if (j < PW_GMIN || j < G) *reinterpret_cast<float4*>(wl + 8 * j + 4 * h) = q[j];
#pragma unroll
                    for (int r = 0; r < PW_TMAX; r++)
                        if (h == 0 && r < R) wl[8 * G + r] = qt[r];
                }
                wave_sync();
            }
            // four entries per lane (jlo, jhi and V = VP are 0 mod 4 here): one action, two 8-byte window
            // reads (a category starts at 2 mod 4), one 16-byte P and one 8-byte slot store; the same
            // expressions per entry, ascending j within the lane
            for (int j = jlo + 4 * lane; quad && j < jhi; j += 256) {
                const int ci = j / NCOMB;  // (compact_to_action's 10-dice form)
                const float* w = win + (NBID + NCOMB * (int)((vi.cats >> (4 * ci)) & 0xF) + (j - ci * NCOMB) - wbase);
                const float2 w01 = *reinterpret_cast<const float2*>(w), w23 = *reinterpret_cast<const float2*>(w + 2);
                const float pa4[4] = {w01.x, w01.y, w23.x, w23.y};
                float p4[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const float pa = pa4[u];
                    const float p = sum > 0.0f ? pa / sum : inv_fallback;
                    const float u0 = (d.c32 * p) * sqe0;
                    if (u0 > fb) {
                        fb = u0;
                        fj = j + u;
                    }
                    p4[u] = p;
                }
                *reinterpret_cast<float4*>(P + j) = make_float4(p4[0], p4[1], p4[2], p4[3]);
                *reinterpret_cast<uint2*>(S + j) = make_uint2(0u, 0u);
            }
            for (int j0 = jlo + lane; !quad && j0 < jhi; j0 += 256) {  // four gathers in flight per lane
                float xa[4];
                int aa[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int j = j0 + 64 * u;
                    aa[u] = j < V ? compact_to_action(vi, j) : 0;
                    xa[u] = (d.prior == 0 && !fast && !staged && j < V) ? xr[aa[u]] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int j = j0 + 64 * u;
                    if (j < jhi) {
                        float p = 0.0f;
                        if (j < V) {
                            const float pa = (fast || staged) ? win[wslot(aa[u])]
                                             : d.prior == 0   ? softmax_p(xa[u], mx, lse)
                                                              : hash_prior_pi(hsh, aa[u]);
                            p = sum > 0.0f ? pa / sum : inv_fallback;
                            const float u0 = (d.c32 * p) * sqe0;
                            if (u0 > fb) {  // ascending j within the lane: strict '>' keeps the lowest
                                fb = u0;
                                fj = j;
                            }
                        }
                        P[j] = p;
                        S[j] = 0;
                    }
                }
            }
            }
            wave_argmax_step(fb, fj);  // the largest u0, the lowest index among equals
            if (lane == 0) {
                NodeRec r;
#pragma unroll
                for (int i = 0; i < 8; i++) r.key[i] = s.w[i];
                r.hash = ihsh;
                r.vinfo = pack_vinfo(vi);
                r.p_off = off;
                r.nvalid = (uint32_t)V;
                r.Ns = 0;
                r.first_j = (uint32_t)fj;
                d.nodes[g][(long)t * d.NCAP + nid] = r;
                if (!insert_index(d, g, t, ihsh, nid)) atomicOr(d.err, ERR_HASH);
            }
            end_id = nid + 1;
            if (lane == 0) {
                d.node_count[g * d.T + t] = nid + 1;
                d.arena_top[t] = off + (uint32_t)VP;
                unsigned long long* gs = reinterpret_cast<unsigned long long*>(d.gstats + (long)e * GST);
                atomicAdd(gs + 0, 1ull);
                atomicAdd(gs + 3, (unsigned long long)V);
                atomicAdd(gs + (fast == 1 ? 9 : fast == 2 ? 10 : 11), 1ull);  // the prior's path
                atomicMax(gs + 4, (unsigned long long)(nid + 1));
                atomicMax(gs + 6, (unsigned long long)(off + (uint32_t)VP));
            }
        }
        res = PyV{-(double)v, T_F32};  // return -v  (MCTS.py:115)
    } else {
        end_id = d.end_node[e];
    }
    // ---- backup (MCTS.py:154-164): the path's nodes are distinct, so every level updates in
    // parallel; level k receives v * (-1)^(depth-1-k) ("return -v" per level).
    const int depth = d.path_len[e];
    if (depth > 0) {
        NodeRec* nodes = d.nodes[g] + (long)t * d.NCAP;
        Edge* edges = d.edges[g] + (long)t * d.ECAP;
        uint16_t* Sb = d.arenaS + (long)t * d.AE;
        const uint64_t* path = d.path + (long)e * MAXD;
        const uint32_t ne0 = d.edge_count[g * d.T + t];
        uint64_t pe = 0;
        uint16_t sl = 0;
        if (lane < depth) {
            pe = path[lane];
            sl = Sb[pe >> 32];
        }
        // the child each level's edge leads to: the next level's node, or for the last edge the
        // node the descent ended at (the new leaf, or a node without valid actions); cached in
        // the edge's tag when that transition drew no dice
        const uint32_t pnext = __shfl((uint32_t)pe, (lane + 1) & 63, 64);
        const uint32_t cnode = lane + 1 < depth ? (pnext & ~PATH_DET) + 1 : end_id;
        const uint32_t cbits = ((uint32_t)pe & PATH_DET) ? cnode << 2 : 0u;
        const bool is_new = lane < depth && sl == 0;
        const uint64_t bal = __ballot(is_new);
        const uint32_t eid = ne0 + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
        const uint32_t ne1 = ne0 + (uint32_t)__popcll(bal);
        if (lane < depth) {
            PyV v = res;
            if ((depth - 1 - lane) & 1) v.v = -v.v;
            if (sl) {
                Edge& ed = edges[sl - 1];
                const PyV q = pv_update(PyV{ed.Q, edge_kind(ed.tag)}, ed.N, v);
                ed.Q = q.v;
                ed.tag = q.t | cbits;
                ed.N += 1;
            } else if (eid < (uint32_t)d.ECAP && eid < 65535u) {
                edges[eid] = Edge{v.v, 1u, v.t | cbits};
                Sb[pe >> 32] = (uint16_t)(eid + 1);
            } else {
                atomicOr(d.err, ERR_EDGES);
            }
            nodes[(uint32_t)pe & ~PATH_DET].Ns += 1;
        }
        if (lane == 0) {
            d.edge_count[g * d.T + t] = ne1;
            atomicMax(reinterpret_cast<unsigned long long*>(d.gstats + (long)e * GST) + 5, (unsigned long long)ne1);
            // a new edge at level 0 (the move's root): into the root's visited list (root_scan)
            if (is_new && eid < (uint32_t)d.ECAP && eid < 65535u) {
                const uint32_t n = d.root_c[2 * t + 1].z;
                if (n != RV_OFF) {
                    const uint32_t j = (uint32_t)(pe >> 32) - d.root_c[2 * t].y;
                    if (n < (uint32_t)RV_CAP) {
                        d.rv[(long)t * RV_CAP + n] = j | ((eid + 1) << 12);
                        d.root_c[2 * t + 1].z = n + 1;
                    } else {
                        d.root_c[2 * t + 1].z = RV_OFF;  // too many: full scans for the rest of the move
                    }
                }
            }
        }
    }
}

// The root's P order for root_scan, once per move after its first expansion (the root is expanded
// by then, by this move's first simulation or an earlier search): the compact set sorted by P
// descending, ascending index on ties (a bitonic sort of 64-bit keys P bits << 32 | 0xFFFF - j in
// LDS; P >= 0, so its bits order as unsigned), and the list of the edges already visited.  One
// workgroup per game.  Leaves the root in full-scan mode when c <= 0 (the order is then not the
// UCB order), when the root has at most 256 valid actions (every bid node), or when its visited
// list would overflow.
__global__ __launch_bounds__(256) void k_root_sort(EngDev d) {
    constexpr int PT = (RO_CAP + 255) / 256;  // keys per thread
    __shared__ uint64_t sk[RO_K];
    __shared__ uint32_t hist[256];
    __shared__ int s_nid, s_need;
    __shared__ uint32_t s_nv, s_cnt;
    __shared__ uint64_t s_prefix;
    const int e = d.e_lo + (int)blockIdx.x;
    if (e >= d.e_hi || d.done[e] || d.idle[e] || !(d.c32 > 0.f)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int t = tree_of(d, e);
    const int g = d.gen[t];
    const uint4 rc0 = d.root_c[2 * t];
    if (tid < 64) {
        int nid = rc0.x ? (int)rc0.x - 1 : -1;
        if (nid < 0) {
            const YkS r = ld_state(d.root + e);
            nid = lookup(d, g, t, r, index_hash(r));
        }
        if (tid == 0) {
            s_nid = nid;
            s_nv = 0;
            s_cnt = 0;
        }
    }
    __syncthreads();
    const int nid = s_nid;
    if (nid < 0) return;
    const NodeRec& nd = d.nodes[g][(long)t * d.NCAP + nid];
    const int V = (int)nd.nvalid;
    const uint32_t p_off = nd.p_off;
    // (a root of <= 256 entries is one pass of the full scan, 4 entries per lane: no order pays)
    if (V <= 256 || V > RO_CAP) return;
    const float* P = d.arenaP + (long)t * d.AE + p_off;
    const uint16_t* S = d.arenaS + (long)t * d.AE + p_off;
    uint32_t* rv = d.rv + (long)t * RV_CAP;
    // keys P bits << 16 | (0xFFFF - j): unique, ordered as (P descending, j ascending); 0 = no entry
    uint64_t key[PT];
#pragma unroll
    for (int i = 0; i < PT; i++) {
        const int j = tid + 256 * i;
        key[i] = 0;
        if (j < V) {
            key[i] = ((uint64_t)__float_as_uint(P[j]) << 16) | (uint32_t)(0xFFFFu - (uint32_t)j);
            const uint16_t sl = S[j];
            if (sl) {
                const uint32_t pos = atomicAdd(&s_nv, 1u);
                if (pos < (uint32_t)RV_CAP) rv[pos] = (uint32_t)j | ((uint32_t)sl << 12);
            }
        }
    }
    const int K = V < d.ro_k ? V : d.ro_k;
    uint64_t thr = 1;  // the keys >= thr are the top K
    if (V > K) {  // radix select of the K-th largest key, 8 bits at a time from the top of 48
        uint64_t prefix = 0, mask = 0;
        int need = K;
        for (int sh = 40; sh >= 0; sh -= 8) {
            hist[tid] = 0;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PT; i++)
                if (key[i] && (key[i] & mask) == prefix) atomicAdd(&hist[(uint32_t)(key[i] >> sh) & 255u], 1u);
            __syncthreads();
            if (tid < 64) {  // the bin holding the need-th largest: suffix sums over lanes of 4 bins each
                const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
                const uint32_t own = h0 + h1 + h2 + h3;
                uint32_t suf = own;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t x = __shfl_down(suf, o, 64);
                    if (lane + o < 64) suf += x;
                }
                const uint32_t above = suf - own;
                if (above < (uint32_t)need && (uint32_t)need <= suf) {
                    const uint32_t hb[4] = {h0, h1, h2, h3};
                    uint32_t c = above;
                    int b = 3;
                    for (; b > 0; b--) {
                        if (c + hb[b] >= (uint32_t)need) break;
                        c += hb[b];
                    }
                    s_prefix = prefix | ((uint64_t)(4 * lane + b) << sh);
                    s_need = need - (int)c;
                }
            }
            __syncthreads();
            prefix = s_prefix;
            need = s_need;
            mask |= (uint64_t)255 << sh;
        }
        thr = prefix;
    }
#pragma unroll
    for (int i = 0; i < PT; i++)
        if (key[i] && key[i] >= thr) sk[atomicAdd(&s_cnt, 1u)] = key[i];
    int n2 = 64;
    while (n2 < K) n2 <<= 1;
    __syncthreads();
    for (int i = K + tid; i < n2; i += 256) sk[i] = 0;  // padding sorts last
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1) {  // bitonic sort, descending
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2 / 2; i += 256) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t a = sk[lo], b = sk[hi];
                if ((a < b) == desc) {
                    sk[lo] = b;
                    sk[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    uint16_t* oj = d.ro_j + (long)t * RO_K;
    float* op = d.ro_p + (long)t * RO_K;
    for (int i = tid; i < K; i += 256) {
        const uint64_t k = sk[i];
        oj[i] = (uint16_t)(0xFFFFu - (uint32_t)(k & 0xFFFFu));
        op[i] = __uint_as_float((uint32_t)(k >> 16));
    }
    if (tid == 0) {  // the next descent need not look the root up; .w: the order's stored entries
        d.root_c[2 * t] = make_uint4((uint32_t)nid + 1, p_off, (uint32_t)V, (uint32_t)K);
        d.root_c[2 * t + 1] = make_uint4((uint32_t)nd.vinfo, (uint32_t)(nd.vinfo >> 32),
                                         s_nv <= (uint32_t)RV_CAP ? s_nv : RV_OFF, 0);
    }
}

// getActionProb tail (MCTS.py:40-54) + Coach sampling/step (Coach.py:59-72).  One wave per game.
// kind: 0, or YK_REC_FAST for a fast move of the playout cap (ORed into the record's status word).
// PRUNE (a full self-play move with forced playouts and pruning on): the gathered list is
// pruned in LDS before it is recorded and drawn from - the tree keeps its raw N and Q, info[4] the raw Ns.
// TEMPER (a move the move-selection temperature applies to, DESIGN.md s6h: a temp-1 move of self-play whose
// T is not 1): the move is drawn from N^(1/T) over the same list, by the whole wave (wave_temper_pick,
// yk_temper.h), with the one uniform the temp-1 draw takes; everything else, the record included, is as without.
template <class... FD>  // (as k_select's: ForcedDev for PRUNE, then TemperDev for TEMPER)
__global__ __launch_bounds__(256) void k_move_end(EngDev d, int move, int kind, FD... fdp) {
    static_assert(yk::args_in(yk::Args<ForcedDev, TemperDev>{}, yk::Args<FD...>{}), "ForcedDev, then TemperDev, no further argument");
    constexpr bool PRUNE = yk::has_arg<ForcedDev, FD...>, TEMPER = yk::has_arg<TemperDev, FD...>;
    const ForcedDev fd = yk::opt_arg(ForcedDev{0.0, 0.0}, fdp...);
    __shared__ uint32_t vis_all[GAMES_PER_BLOCK][ASIZE];
    __shared__ double stage_all[TEMPER ? GAMES_PER_BLOCK : 1][TEMPER ? 64 : 1];  // wave_temper_pick's pieces of 64 terms
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e = d.e_lo + blockIdx.x * GAMES_PER_BLOCK + w;
    if (e >= d.e_hi) return;
    if (d.done[e]) return;
    uint32_t* vis = vis_all[w];
    const int t = tree_of(d, e);  // before the real step changes cur
    const int g = d.gen[t];
    const YkS r = ld_state(d.root + e);
    const bool idle = d.idle[e] != 0;
    const int nid = idle ? -1 : lookup(d, g, t, r, index_hash(r));
    int nvis = 0;
    uint32_t root_ns = 0xFFFFFFFFu;
    if (idle) {
    } else if (nid >= 0) {
        const NodeRec& nd = d.nodes[g][(long)t * d.NCAP + nid];
        root_ns = nd.Ns;
        const VInfo vi = unpack_vinfo(nd.vinfo, nd.nvalid);
        const uint16_t* S = d.arenaS + (long)t * d.AE + nd.p_off;
        const Edge* edges = d.edges[g] + (long)t * d.ECAP;
        // 8 pieces of 64 entries at a time: their slot loads, then their edge loads, all in flight
        // together (one round trip each per 512 entries instead of per 64)
        constexpr int MB = 8;
        const int nv = (int)nd.nvalid;
        for (int j0 = 0; j0 < nv; j0 += 64 * MB) {
            uint16_t sl[MB];
#pragma unroll
            for (int b = 0; b < MB; b++) {
                const int j = j0 + 64 * b + lane;
                const uint16_t x = S[j < nv ? j : 0];  // unconditional loads (in bounds): no wait at a branch join
                sl[b] = j < nv ? x : 0;
            }
            uint32_t n[MB];
#pragma unroll
            for (int b = 0; b < MB; b++) {
                const uint32_t x = edges[sl[b] ? sl[b] - 1 : 0].N;
                n[b] = sl[b] ? x : 0u;
            }
#pragma unroll
            for (int b = 0; b < MB; b++) {
                const int j = j0 + 64 * b + lane;
                const uint64_t bal = __ballot(sl[b] != 0);
                if (sl[b]) {
                    const int pos = nvis + __popcll(bal & ((1ull << lane) - 1));
                    // (PRUNE: the compact index for now - the pruning needs the edge's P and slot)
                    vis[pos] = ((uint32_t)(PRUNE ? j : compact_to_action(vi, j)) << 16) | (n[b] & 0xFFFF);
                }
                nvis += __popcll(bal);
            }
        }
        if (PRUNE && nvis > 0) {
            // policy target pruning: lanes stride the visited edges.  The best child c* - the largest N, the
            // lowest action among equals (the list ascends in action) - keeps its count and sets the bound
            const float* P = d.arenaP + (long)t * d.AE + nd.p_off;
            wave_sync();
            int bn = -1, bi = 0x7FFFFFFF;
            for (int i = lane; i < nvis; i += 64) {
                const int c = (int)(vis[i] & 0xFFFF);
                if (c > bn) {
                    bn = c;
                    bi = i;
                }
            }
            wave_argmax_step(bn, bi);
            const int jb = (int)(vis[bi] >> 16);
            const Edge eb = edges[S[jb] - 1];
            const double pstar = puct_value(eb.Q, P[jb], root_ns, fd.c, eb.N);
            // every other edge's pruned count; the edges left without a visit leave the list, which is
            // compacted in place a piece of 64 at a time (a piece is read whole before any of it is written,
            // and the writes land at or before the entries read)
            int out = 0;
            uint32_t cut = 0;
            for (int i0 = 0; i0 < nvis; i0 += 64) {
                const int i = i0 + lane;
                uint32_t word = 0;
                bool keep = false;
                if (i < nvis) {
                    const int j = (int)(vis[i] >> 16);
                    const Edge ev = edges[S[j] - 1];
                    const uint32_t n = i == bi ? ev.N : pruned_count(ev.N, ev.Q, P[j], root_ns, fd.k, fd.c, pstar);
                    cut += ev.N - n;
                    keep = n > 0;
                    word = ((uint32_t)compact_to_action(vi, j) << 16) | (n & 0xFFFF);
                }
                const uint64_t bal = __ballot(keep);
                wave_sync();
                if (keep) vis[out + __popcll(bal & ((1ull << lane) - 1))] = word;
                out += __popcll(bal);
            }
            nvis = out;
            cut = (uint32_t)xlane_sum((int)cut);
            if (lane == 0 && cut)
                atomicAdd(reinterpret_cast<unsigned long long*>(d.gstats + (long)e * GST) + 13, (unsigned long long)cut);
        }
    } else if (lane == 0) {
        atomicOr(d.err, ERR_ROOT);
    }
    // GreedyYachtPlayer's heuristic needs the whole wave (YachtPlayers.py:186-214)
    int gact = -1;
    if (idle && (d.cur[e] == d.seat[e] ? d.arena_agent : d.arena_opp) == YK_PLAYER_GREEDY)
        gact = greedy_heuristic_wave(r, lane);
    wave_sync();
    // record the visit counts (sparse, ascending action)
    const long vbase = (long)e * d.VCAP;
    const int voff = d.rec_voff[(long)e * (d.M + 1) + move];
    const bool room = voff + nvis <= d.VCAP;
    if (room)
        for (int i = lane; i < nvis; i += 64) d.rec_visits[vbase + voff + i] = vis[i];
    // the tempered draw needs the whole wave; every lane takes the same uniform from its own copy of the
    // stream, and lane 0 below advances the game's by that one draw
    int tpick = -1;
    double ttotal = 0.0;
    if constexpr (TEMPER) {
        if (!idle && !d.arena && move + 1 < d.temp_threshold) {  // (wave-uniform) a temp-1 move, as below
            Stream ru{d.seed, d.env_id[e], d.ctr[e]};
            const double u = ru.uniform53();
            tpick = wave_temper_pick([&](int i) { return vis[i] & 0xFFFF; }, nvis, 1.0 / yk::get_arg<TemperDev>(fdp...).move_t[move],
                                     u, stage_all[w], lane, &ttotal);
        }
    }
    if (lane != 0) return;
    if (!room) atomicOr(d.err, ERR_VISITS);
    d.rec_voff[(long)e * (d.M + 1) + move + 1] = room ? voff + nvis : voff;
    const int stepi = move + 1;
    const int temp = d.arena ? 0 : (stepi < d.temp_threshold ? 1 : 0);  // Coach.py:58
    Stream rs{d.seed, d.env_id[e], d.ctr[e]};
    int action = 0;
    if (idle && gact >= 0) {
        action = gact;  // the greedy heuristic's (valid) choice
    } else if (idle) {
        // RandomYachtPlayer.play, and GreedyYachtPlayer's fallback: np.random.choice over the
        // ascending legal actions of the canonical board (YachtPlayers.py:174-183, 204-214);
        // no legal action -> 0 without a draw
        const VInfo vi = valid_info(r, 1);
        if (vi.V > 0) action = compact_to_action(vi, rs.below(vi.V));
    } else if (temp == 0) {
        // bestAs = argwhere(counts == max(counts)); np.random.choice(bestAs)  (MCTS.py:44-49)
        uint32_t mx = 0;
        for (int i = 0; i < nvis; i++) mx = max(mx, vis[i] & 0xFFFF);
        if (mx == 0) {
            action = rs.below(ASIZE);  // every count is 0: all 3226 actions tie
        } else {
            int nb = 0;
            for (int i = 0; i < nvis; i++) nb += (vis[i] & 0xFFFF) == mx;
            int pick = rs.below(nb);
            for (int i = 0; i < nvis; i++)
                if ((vis[i] & 0xFFFF) == mx && pick-- == 0) {
                    action = (int)(vis[i] >> 16);
                    break;
                }
        }
        // np.random.choice(len(pi), p=one-hot) still draws in Coach (Coach.py:65); the Arena
        // agent is np.argmax(pi) (Coach.py:124-125), which does not
        if (!d.arena) (void)rs.uniform53();
    } else if (TEMPER) {
        // the wave drew above from N^(1/T): the same single uniform, the same error when there is nothing to draw from
        if (!(ttotal > 0.0)) {
            atomicOr(d.err, ERR_ZERO_COUNTS);
        } else {
            (void)rs.uniform53();
            action = tpick >= 0 ? (int)(vis[tpick] >> 16) : ASIZE;
        }
    } else {
        // probs = counts / sum; np.random.choice(len(pi), p=probs): cumsum, /= cdf[-1],
        // searchsorted(u, 'right')
        double total = 0.0;
        for (int i = 0; i < nvis; i++) total += (double)(vis[i] & 0xFFFF);
        if (total == 0.0) {
            atomicOr(d.err, ERR_ZERO_COUNTS);
        } else {
            double c = 0.0;
            for (int i = 0; i < nvis; i++) c += (double)(vis[i] & 0xFFFF) / total;
            const double last = c;
            const double u = rs.uniform53();
            c = 0.0;
            action = ASIZE;
            for (int i = 0; i < nvis; i++) {
                c += (double)(vis[i] & 0xFFFF) / total;
                if (c / last > u) {
                    action = (int)(vis[i] >> 16);
                    break;
                }
            }
        }
    }
    // record + real step (Coach.py:61-67)
    const long ri = (long)e * d.M + move;
    st_state(d.rec_state + ri, r);
    d.rec_ctr[ri * 2 + 1] = rs.ctr;
    const int player = d.cur[e];
    YkS b = ld_state(d.board + e);
    int np = 0;
    const int st = step_state(b, player, action, rs, np);
    int32_t* info = d.rec_info + ri * 8;
    info[0] = temp;
    info[1] = player;
    info[2] = action;
    info[3] = (int32_t)d.gstats[(long)e * GST + 0];
    info[4] = (int32_t)root_ns;
    info[5] = nvis;
    info[6] = st | kind;
    info[7] = 0;
    d.nmoves[e] = stepi;
    if (st != YK_ST_OK) {
        atomicOr(d.err, ERR_STEP);
        d.done[e] = 1;
        return;
    }
    st_state(d.board + e, b);
    d.cur[e] = np;
    d.ctr[e] = rs.ctr;
    const double rgame = game_ended(b, np);  // Coach.py:69
    if (rgame != 0.0) {
        d.done[e] = 1;
        d.final_r[e] = rgame;
        d.final_cur[e] = np;
        d.final_tot[2 * e] = total_with_bonus(b, 0);
        d.final_tot[2 * e + 1] = total_with_bonus(b, 1);
    } else if (stepi >= d.M) {
        atomicOr(d.err, ERR_MOVES);
        d.done[e] = 1;
        d.final_r[e] = 0.0;
        d.final_cur[e] = np;
    }
}

// example values r * (-1)**(player != curPlayer)  (Coach.py:71-72)
__global__ void k_finalize(EngDev d) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)d.E * d.M) return;
    const int e = (int)(t / d.M), m = (int)(t % d.M);
    if (m >= d.nmoves[e]) {
        d.rec_val[t] = 0.0;
        return;
    }
    const int pl = d.rec_info[t * 8 + 1];
    d.rec_val[t] = d.final_r[e] * ((pl != d.final_cur[e]) ? -1.0 : 1.0);
}

// dense root visit counts for the MCTS plugin (MCTS.py:41-42)
__global__ void k_root_counts(EngDev d, int32_t* counts) {
    const int lane = threadIdx.x & 63;
    const int e = d.e_lo + blockIdx.x * GAMES_PER_BLOCK + (threadIdx.x >> 6);
    if (e >= d.e_hi) return;
    int32_t* c = counts + (long)e * ASIZE;
    for (int a = lane; a < ASIZE; a += 64) c[a] = 0;
    wave_sync();
    const int g = d.gen[e];
    const YkS r = ld_state(d.root + e);
    const int nid = lookup(d, g, e, r, index_hash(r));
    if (nid < 0) return;
    const NodeRec& nd = d.nodes[g][(long)e * d.NCAP + nid];
    const VInfo vi = unpack_vinfo(nd.vinfo, nd.nvalid);
    const uint16_t* S = d.arenaS + (long)e * d.AE + nd.p_off;
    const Edge* edges = d.edges[g] + (long)e * d.ECAP;
    for (int j = lane; j < (int)nd.nvalid; j += 64)
        if (S[j]) c[compact_to_action(vi, j)] = (int32_t)edges[S[j] - 1].N;
}

__global__ void k_count_done(const uint8_t* done, int E, int32_t* out) {
    __shared__ int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    int c = 0;
    for (int e = threadIdx.x; e < E; e += blockDim.x) c += done[e] ? 1 : 0;
    atomicAdd(&s, c);
    __syncthreads();
    if (threadIdx.x == 0) *out = s;
}

}  // namespace

// ------------------------------------------------------------------ host object
struct yk_engine {
    yk_engine_config_t cfg;
    yk_net_t* net = nullptr;
    yk_net_t* net2 = nullptr;  // the opponent seat's net with dual trees (default: net)
    // dual trees, one game group, row tiles x head parts x 2 <= CUs: the opponent seat's forward
    // runs on its own stream beside the agent's (disjoint rows), with fparts_dual head parts
    hipStream_t dstream = nullptr;
    hipEvent_t ev_d0 = nullptr, ev_d1 = nullptr;
    int fparts_single = 1, fparts_dual = 0;  // fparts_dual 0: the two forwards stay in sequence
    EngDev d{};
    DeviceBlocks mem;  // every device array below and in d / nz
    float* logits = nullptr;
    float* vpred = nullptr;
    float2* mlse = nullptr;
    float *lut_sq = nullptr, *lut_sqe = nullptr;
    int32_t* done_count = nullptr;
    int32_t* host_done = nullptr;
    uint32_t* mcts_env = nullptr;
    bool have_records = false;
    bool have_arena = false;
    // game groups: the batch is split into `ngroups` ranges, each on its own
    // stream, so one group's forward runs beside another group's expand
    int ngroups = 1;
    hipStream_t gs[YK_MAX_GROUPS] = {};
    hipEvent_t ev_fork = nullptr, ev_join[YK_MAX_GROUPS] = {}, ev_fwd[YK_MAX_GROUPS] = {};
    // profiling (yk_engine_profile): per-kernel-class HIP events on each group's stream; the
    // forward / expand pair is timed in every prof_stride-th simulation (an event record between
    // two dependent launches costs ~4 us of GPU time, so timing every one slows the batch ~5 %)
    bool prof = false;
    int prof_stride = 1;
    struct ProfLog {
        std::vector<hipEvent_t> ev;
        std::vector<int> cls;
        int used = 0;
    } pg[YK_MAX_GROUPS];
    double kms[8] = {0};
    int64_t klaunch[8] = {0};
    bool root_scan = true;  // the incremental root scan (k_root_sort + root_scan); YK_ROOT_SCAN=0: full scans
    bool split_descent = false;  // YK_SPLIT_DESCENT=1: the descent as its own k_select launch (same trees)
    NoiseDev nz{};               // Dirichlet root noise of yk_selfplay (configured: alpha > 0 and eps > 0)
    bool noise = false;
    bool have_priors = false;    // the last batch was a self-play batch with noise: yk_engine_root_priors
    bool root_values = false;    // record_root_values: k_root_value after each k_move_end of yk_selfplay
    int fast_sims = 0;           // playout cap (yk_engine_set_playout_cap; 0: off): a fast move's simulations
    double full_prob = 1.0;      // and the probability that a move of a yk_selfplay batch is a full one
    int64_t fast_moves = 0;      // lock-step moves of the last batch that ran with the fast cap
    double forced_k = 0.0;       // forced playouts (yk_engine_set_forced_playouts; 0: off) at the self-play roots
    bool forced_prune = true;    // of full moves, and whether k_move_end prunes the move's counts
    bool util_on = false;        // the score-margin utility (yk_engine_set_score_utility) at the
    double util_w = 0.0, util_c = 1.0;  // terminal states of every search of this engine: the weight and the scale
    unsigned long long* util_terminals = nullptr;  // [E] terminal descents that returned a utility (counter 9)
    bool fpu_on = false;         // first-play urgency (yk_engine_set_fpu) in every search of this
    double fpu_r = 0.0, fpu_r_root = 0.0;  // engine: the reduction at interior nodes and at depth 0
    // the self-play temperatures (yk_engine_set_temperatures): each schedule's T by move, M
    // entries, on the host (which picks each move's instantiation from it) and on the device (which reads T)
    bool move_temp = false, root_temp = false;
    std::vector<double> move_t, root_t;
    TemperDev td{nullptr, nullptr};
    double *dev_move_t = nullptr, *dev_root_t = nullptr;
    yk_engine() = default;
    yk_engine(const yk_engine&) = delete;
    yk_engine& operator=(const yk_engine&) = delete;
    ~yk_engine() {  // (also of a half-made engine: yk_engine_create's early returns)
        for (auto& L : pg)
            for (hipEvent_t e : L.ev) (void)hipEventDestroy(e);
        for (int g = 0; g < YK_MAX_GROUPS; g++) {
            if (gs[g]) (void)hipStreamDestroy(gs[g]);
            if (ev_join[g]) (void)hipEventDestroy(ev_join[g]);
            if (ev_fwd[g]) (void)hipEventDestroy(ev_fwd[g]);
        }
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (dstream) (void)hipStreamDestroy(dstream);
        if (ev_d0) (void)hipEventDestroy(ev_d0);
        if (ev_d1) (void)hipEventDestroy(ev_d1);
        if (host_done) (void)hipHostFree(host_done);
    }
};

namespace {
// kernel classes for yk_engine_kernel_times
enum { KC_SELECT = 0, KC_FORWARD = 1, KC_SCAN = 2 /* k_root_sort + the second descent */, KC_EXPAND = 3, KC_MOVE_BEGIN = 4, KC_MOVE_END = 5, KC_NOISE = 6 /* k_root_noise, both phases */, KC_ROOT_VALUE = 7 /* k_root_value */, KC_N = 8 };

void prof_mark(yk_engine* eng, int g, int cls, hipStream_t s) {  // records an event pair boundary
    if (!eng->prof) return;
    auto& L = eng->pg[g];
    if (L.used + 1 >= (int)L.ev.size()) {
        const size_t old = L.ev.size();
        L.ev.resize(old + 4096);
        L.cls.resize(old + 4096);
        for (size_t i = old; i < L.ev.size(); i++) (void)hipEventCreate(&L.ev[i]);
    }
    L.cls[L.used] = cls;
    (void)hipEventRecord(L.ev[L.used++], s);
}
void prof_collect(yk_engine* eng) {  // call after a stream sync
    if (!eng->prof) return;
    for (int g = 0; g < eng->ngroups; g++) {
        auto& L = eng->pg[g];
        for (int i = 0; i + 1 < L.used; i++) {
            const int cls = L.cls[i];
            if (cls < 0) continue;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, L.ev[i], L.ev[i + 1]) == hipSuccess) {
                eng->kms[cls] += ms;
                eng->klaunch[cls] += 1;
            }
        }
        L.used = 0;
    }
}

// the device view of group g (its game range)
EngDev group_dev(const yk_engine* eng, int g) {
    EngDev d = eng->d;
    const int G = eng->ngroups;
    auto bound = [&](int k) {
        const long b = (long)d.E * k / G;
        return k == G ? d.E : (int)std::min<long>(d.E, (b + GROUP_ALIGN - 1) / GROUP_ALIGN * GROUP_ALIGN);
    };
    d.e_lo = bound(g);
    d.e_hi = bound(g + 1);
    return d;
}
dim3 game_grid(const EngDev& d) {
    return dim3((unsigned)std::max(1, (d.e_hi - d.e_lo + GAMES_PER_BLOCK - 1) / GAMES_PER_BLOCK));
}

int check_errors(yk_engine* eng, hipStream_t s) {
    uint32_t err = 0;
    uint32_t nerr[2] = {0u, 0u};
    YK_HIP(hipMemcpyAsync(&err, eng->d.err, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (eng->net) YK_HIP(hipMemcpyAsync(&nerr[0], eng->net->dev.err, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (eng->net2) YK_HIP(hipMemcpyAsync(&nerr[1], eng->net2->dev.err, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    YK_HIP(hipStreamSynchronize(s));
    if ((nerr[0] | nerr[1]) && !(err & ERR_FWD_SYNC)) {  // into the engine's word, so yk_engine_stats shows it
        err |= ERR_FWD_SYNC;
        YK_HIP(hipMemcpy(eng->d.err, &err, sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (err & (ERR_NODES | ERR_EDGES | ERR_ARENA | ERR_DEPTH | ERR_VISITS | ERR_HASH)) return YK_ERR_CAPACITY;
    if (err) return YK_ERR_STATE;
    return YK_OK;
}
// `sims` simulations for every game of groups 0 .. G-1, group g on stream st[g].  Within a group
// (and a game) the simulations are sequential; the groups' streams run free, so a forward runs
// beside the other groups' expand.  (Staggering them - group g's forward k waiting for group
// g-1's forward k through an event; at 8192 games x 2 groups that costs 1.2 %,
// profiles/r02h_stagger_ab.log.)
// noise_move >= 0 (self-play with root noise): that move's roots are noised - k_root_noise phase 0
// before the first descent, phase 1 after simulation 0's expansion, which then ends without the
// fused descent whatever the root-scan mode.  -1: no noise launch is made.
// forced (a full self-play move with forced playouts): the descents are the FORCED
// instantiations; every other caller runs the unforced ones, whose code the feature leaves as it was.
// Whether they are the FPU ones is the engine's state (yk_engine_set_fpu), the same for every caller; so is
// whether they are the score-margin utility's (yk_engine_set_score_utility).
// root_t (a self-play move under the root policy temperature, DESIGN.md s6h: the device table of T by move):
// the two launches of noise_move are the tempered forms of k_root_noise - with `with_noise` the one that also
// mixes the noise, else the one without the sampler.  NULL: the launches are the noise's own, as before.
int run_sims(yk_engine* eng, int G, const hipStream_t* st, int sims, const uint32_t* env_ids, uint64_t* ctr,
             int noise_move = -1, const ForcedDev* forced = nullptr, const double* root_t = nullptr,
             bool with_noise = true) {
    const dim3 bb(256);
    if (sims <= 0) return YK_OK;
    // first-play urgency: every search of an engine it is set on runs the FPU instantiations
    // the descents' options (yk_optarg.h): the values of those that are on are the kernels' packs
    const auto o_forced = yk::opt(forced != nullptr, forced ? *forced : ForcedDev{0.0, 0.0});
    const auto o_fpu = yk::opt(eng->fpu_on, FpuDev{eng->fpu_r, eng->fpu_r_root});
    const auto o_util = yk::opt(eng->util_on, UtilDev{1.0 - eng->util_w, eng->util_w, eng->util_c, eng->util_terminals});
    const auto select = [&](const EngDev& dd, hipStream_t s) {
        yk::with_opts([&](const auto&... o) {
            hipLaunchKernelGGL((k_select<std::decay_t<decltype(o)>...>), game_grid(dd), bb, 0, s, dd, env_ids, ctr, o...);
        }, o_forced, o_fpu, o_util);
    };
    const auto expand_backup = [&](const EngDev& dd, hipStream_t s, int do_select) {
        yk::with_opts([&](const auto&... o) {
            hipLaunchKernelGGL((k_expand_backup<std::decay_t<decltype(o)>...>), game_grid(dd), bb, 0, s, dd, do_select, env_ids,
                               ctr, o...);
        }, o_forced, o_fpu, o_util);
    };
    const auto root_noise = [&](const EngDev& dd, hipStream_t s, int phase) {
        return root_t ? yk_launch_root_temper(&dd, sizeof(dd), &eng->nz, sizeof(eng->nz), root_t, with_noise ? 1 : 0,
                                              noise_move, phase, s)
                      : yk_launch_root_noise(&dd, sizeof(dd), &eng->nz, sizeof(eng->nz), noise_move, phase, s);
    };
    EngDev dg[YK_MAX_GROUPS];
    for (int g = 0; g < G; g++) {
        dg[g] = G == 1 ? eng->d : group_dev(eng, g);
        if (noise_move >= 0) {  // the roots already in the tree
            prof_mark(eng, g, KC_NOISE, st[g]);
            const int rc = root_noise(dg[g], st[g], 0);
            if (rc) return rc;
        }
        prof_mark(eng, g, KC_SELECT, st[g]);  // the first descent; later ones run in k_expand_backup's tail
        select(dg[g], st[g]);
        YK_LAUNCHED();
    }
    for (int k = 0; k < sims; k++) {
        const bool timed = k % eng->prof_stride == 0;  // sim 0 always: it closes the select interval
        for (int g = 0; g < G; g++) {
            const EngDev& d = dg[g];
            if (d.prior == 0) {
                if (timed) prof_mark(eng, g, KC_FORWARD, st[g]);
                // predict row = game: no compaction; workgroups without a leaf exit at once
                // (dual trees: the agent's leaves on its net, then the opponent's on its own)
                const int lo = d.e_lo;
                const bool conc = d.dual && eng->dstream && G == 1;
                if (conc) {  // the opponent's forward waits for this stream's last expand only
                    YK_HIP(hipEventRecord(eng->ev_d0, st[g]));
                    YK_HIP(hipStreamWaitEvent(eng->dstream, eng->ev_d0, 0));
                }
                for (int side = 0; side < (d.dual ? 2 : 1); side++) {
                    const yk_net_t* net = side ? eng->net2 : eng->net;
                    hipStream_t fs = conc && side == 1 ? eng->dstream : st[g];
                    int rc = launch_forward(net->dev, d.leaf_state + lo, nullptr, nullptr, nullptr, d.e_hi - lo,
                                            eng->logits + (size_t)lo * PI_LD, eng->vpred + lo, fs,
                                            d.leaf_flag + lo, eng->mlse + lo, true, d.dual ? (uint8_t)(1u << side) : 0xFF,
                                            d.fparts, d.E);
                    if (rc) return rc;
                }
                if (conc) {
                    YK_HIP(hipEventRecord(eng->ev_d1, eng->dstream));
                    YK_HIP(hipStreamWaitEvent(st[g], eng->ev_d1, 0));
                }
            }
            if (timed) prof_mark(eng, g, KC_EXPAND, st[g]);
            // the move's first expansion ends without the next descent: the root's P order is built
            // in between (k_root_sort; root_scan uses it for the move's remaining simulations)
            const bool sort_root = k == 0 && sims > 1 && eng->root_scan;
            const bool noise = k == 0 && noise_move >= 0;  // the roots simulation 0 has just expanded
            const bool fuse = k + 1 < sims && !sort_root && !noise;  // the next descent in the expand's tail
            expand_backup(d, st[g], fuse && !eng->split_descent ? 1 : 0);
            YK_LAUNCHED();
            if (fuse && eng->split_descent) {
                select(d, st[g]);
                YK_LAUNCHED();
            }
            if (noise) {
                prof_mark(eng, g, KC_NOISE, st[g]);  // (simulation 0 is always a timed one)
                const int rc = root_noise(d, st[g], 1);
                if (rc) return rc;
                if (!sort_root && k + 1 < sims) {  // the second descent on its own, as after k_root_sort
                    prof_mark(eng, g, KC_SCAN, st[g]);
                    select(d, st[g]);
                    YK_LAUNCHED();
                }
            }
            if (sort_root) {
                if (timed) prof_mark(eng, g, KC_SCAN, st[g]);
                hipLaunchKernelGGL(k_root_sort, dim3((unsigned)(d.e_hi - d.e_lo)), bb, 0, st[g], d);
                YK_LAUNCHED();
                select(d, st[g]);
                YK_LAUNCHED();
            }
            if (timed && eng->prof_stride > 1) prof_mark(eng, g, -1, st[g]);  // untimed sims follow
        }
    }
    for (int g = 0; g < G; g++) prof_mark(eng, g, -1, st[g]);
    return YK_OK;
}
}  // namespace

extern "C" {


int yk_engine_create(yk_engine_t** out, const yk_engine_config_t* cfg, yk_net_t* net) {
    if (!out || !cfg) return YK_ERR_ARG;
    if (cfg->n_envs <= 0 || cfg->sims < 1 || cfg->max_moves < 1 || cfg->max_moves > 4096) return YK_ERR_ARG;
    if (cfg->prior == 0 && !net) return YK_ERR_ARG;
    if (cfg->prior != 0 && cfg->prior != 1) return YK_ERR_ARG;
    // root noise: alpha >= 0, eps in [0, 1] (NaN fails both); on when both are > 0
    if (!(cfg->dirichlet_alpha >= 0.0) || !(cfg->dirichlet_eps >= 0.0 && cfg->dirichlet_eps <= 1.0)) return YK_ERR_ARG;
    std::unique_ptr<yk_engine> eng(new yk_engine());  // (owned here until *out is set: every return before frees it)
    eng->cfg = *cfg;
    eng->net = net;
    EngDev& d = eng->d;
    d.E = cfg->n_envs;
    d.sims = cfg->sims;
    d.c32 = (float)cfg->cpuct;
    d.temp_threshold = cfg->temp_threshold;
    d.prior = cfg->prior;
    d.M = cfg->max_moves;
    // capacities: one new node per simulation; a round holds <= 4 real moves
    // and round 2 also keeps the round-2 nodes made while searching round 1 (<= 2 moves).
    d.NCAP = 6 * cfg->sims + 64;
    int hcap = 1;
    while (hcap < 2 * d.NCAP) hcap <<= 1;
    d.HCAP = hcap;
    d.ECAP = std::min(4 * d.NCAP, 65535);
    // Arena: the worst case (every live node a 3024-action score node) cannot overflow; use it
    // when it fits in 60% of free HBM, else a measured-footprint default (overflow is detected).
    if (cfg->arena_entries > 0) {
        d.AE = (cfg->arena_entries + 3) & ~3LL;
    } else {
        const int64_t worst = (int64_t)d.NCAP * 3024;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        const double need = (double)worst * 6.0 * cfg->n_envs * (cfg->dual_trees ? 2 : 1);
        d.AE = (need < 0.6 * (double)free_b) ? worst : (int64_t)cfg->sims * 9000 + 65536;
    }
    d.VCAP = (int)record_vcap(cfg->max_moves, cfg->sims);
    d.rec_pred = cfg->record_predictions ? 1 : 0;
    d.max_exp = cfg->record_predictions ? std::max(cfg->max_expansions, 1) : 0;
    d.rec_stride = std::max(cfg->record_stride, 1);
    d.e_lo = 0;
    d.e_hi = d.E;
    d.T = cfg->dual_trees ? 2 * d.E : d.E;
    d.dual = 0;  // set by yk_arena for MCTS vs MCTS
    eng->net2 = net;
    // game groups: auto = 2 with the net prior at >= 8192 games (the forward of 4096 rows fills the
    // chip in one round, so there a second group's forward beside the first's expand pays: +3.8 %
    // measured), else 1 (below that each simulation is latency-bound: F + X per group does not
    // shrink with the group); each group needs at least one forward row tile
    int G = cfg->groups > 0 ? cfg->groups : ((cfg->prior == 0 && cfg->n_envs >= 8192) ? 2 : 1);
    G = std::max(1, std::min({G, YK_MAX_GROUPS, (cfg->n_envs + GROUP_ALIGN - 1) / GROUP_ALIGN}));
    eng->ngroups = G;
    // forward head split: when a group's row tiles do not fill the CUs, 2 or 4
    // workgroups per tile each take a slice of the policy head (the trunk runs in each)
constexpr int YK_FPARTS_MAX = 4;
    {
        int cus = 256, dev = 0;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        // the G groups' forwards run at once on their own streams: the bound counts every group's
        // tiles (sizing from one group's tiles oversubscribed the chip at G = 4)
        const int tiles = G * (((cfg->n_envs + G - 1) / G + 15) / 16);
        d.fparts = 1;
        while (d.fparts * 2 <= YK_FPARTS_MAX && tiles * d.fparts * 2 <= cus) d.fparts *= 2;
        eng->fparts_single = d.fparts;
        if (cfg->dual_trees && G == 1 && cfg->prior == 0 && 2 * tiles <= cus) {
            eng->fparts_dual = 1;
            while (eng->fparts_dual * 2 <= YK_FPARTS_MAX && 2 * tiles * eng->fparts_dual * 2 <= cus) eng->fparts_dual *= 2;
        }
    }
    const size_t R = ((size_t)cfg->n_envs + d.rec_stride - 1) / d.rec_stride;
    const size_t E = (size_t)d.E, T = (size_t)d.T;
#define A(p, n) YK_TRY(eng->mem.alloc(&(p), (n)))
    for (int g = 0; g < 2; g++) {
        A(d.nodes[g], T * d.NCAP);
        A(d.hidx[g], T * d.HCAP);
        A(d.edges[g], T * d.ECAP);
    }
    A(d.node_count, 2 * T);
    A(d.edge_count, 2 * T);
    A(d.arenaP, T * (size_t)d.AE);
    A(d.arenaS, T * (size_t)d.AE);
    A(d.arena_top, T);
    A(d.gen, T);
    A(d.cur_round, T);
    A(d.root_c, 2 * T);
    A(d.rv, T * RV_CAP);
    A(d.ro_j, T * RO_K);
    A(d.ro_p, T * RO_K);
    A(d.board, E);
    A(d.cur, E);
    A(d.ctr, E);
    A(d.env_id, E);
    A(d.done, E);
    A(d.nmoves, E);
    A(d.root, E);
    A(d.leaf_state, E);
    A(d.leaf_hash, E);
    A(d.leaf_flag, E);
    A(d.path, E * MAXD);
    A(d.path_len, E);
    A(d.end_node, E);
    A(d.res_v, E);
    A(d.res_t, E);
    A(eng->vpred, E);
    A(eng->mlse, E * (size_t)d.fparts);
    A(eng->lut_sq, (size_t)LUT_N);
    A(eng->lut_sqe, (size_t)LUT_N);
    A(d.rec_state, E * d.M);
    A(d.rec_info, E * d.M * 8);
    A(d.rec_ctr, E * d.M * 2);
    A(d.rec_val, E * d.M);
    A(d.rec_visits, E * (size_t)d.VCAP);
    A(d.rec_voff, E * (d.M + 1));
    A(d.final_r, E);
    A(d.final_cur, E);
    A(d.final_tot, 2 * E);
    A(d.seat, E);
    A(d.idle, E);
    A(d.gstats, E * GST);
    A(eng->util_terminals, E);
    YK_HIP(hipMemset(eng->util_terminals, 0, sizeof(unsigned long long) * E));
    A(d.err, 1);
    A(eng->done_count, 1);
    A(eng->mcts_env, E);
    if (d.prior == 0) {
        A(eng->logits, E * (size_t)PI_LD);
    }
    eng->root_values = cfg->record_root_values != 0;
    eng->noise = cfg->dirichlet_alpha > 0.0 && cfg->dirichlet_eps > 0.0;
    eng->nz.alpha = cfg->dirichlet_alpha;
    eng->nz.eps = cfg->dirichlet_eps;
    if (eng->noise) {
        A(eng->nz.noised, E);
        if (d.rec_pred) {
            A(eng->nz.prior_before, R * (size_t)d.M * ASIZE);
            A(eng->nz.prior_after, R * (size_t)d.M * ASIZE);
        }
    }
    if (d.rec_pred) {
        A(d.rec_pi, R * (size_t)d.max_exp * ASIZE);
        A(d.rec_v, R * (size_t)d.max_exp);
        A(d.rec_leaf, R * (size_t)d.max_exp);
    }
#undef A
    if (hipHostMalloc((void**)&eng->host_done, sizeof(int32_t)) != hipSuccess) return YK_ERR_NOMEM;
    {  // YK_ROOT_SCAN=0: every descent scans the root's whole compact set (A/B, and the test that both
       // give the same trees)
        const char* ev = getenv("YK_ROOT_SCAN");
        eng->root_scan = !(ev && ev[0] == '0');
        const char* ek = getenv("YK_ROOT_K");  // a shorter kept order (>= 1): the tests' fallback cases
        d.ro_k = ek ? std::max(1, std::min(RO_K, atoi(ek))) : RO_K;
        // YK_NODE_SUMMARY=0: a node's first scan is a full scan too (A/B, and the test that both give
        // the same trees; the records' first_j is written either way)
        const char* en = getenv("YK_NODE_SUMMARY");
        d.node_summary = (en && en[0] == '0') ? 0 : 1;
        // YK_PRIOR_FAST=0: every leaf's prior takes the dense pass and the gather P write (A/B, and the
        // test that all levels give the same trees); 1: the compact-first paths, general leaves unstaged;
        // 2: those and the staged P write of the general leaves (dense pass kept); unset or anything else (3): a
        // general leaf's priors at 10 dice are also computed compact-first, through the window, four per lane
        const char* ep = getenv("YK_PRIOR_FAST");
        d.prior_fast = (ep && ep[0] >= '0' && ep[0] <= '2' && !ep[1]) ? ep[0] - '0' : 3;
        // YK_SPLIT_DESCENT=1 (measurement): k_expand_backup stops after the backup and each next
        // descent is its own k_select launch, so rocprofv3 times and counts the expansion + backup
        // and the descent apart (the same work: the trees are identical)
        const char* es = getenv("YK_SPLIT_DESCENT");
        eng->split_descent = es && es[0] == '1';
    }
    // (these report YK_ERR_HIP without recording the HIP error)
    if (G > 1) {
        if (hipEventCreateWithFlags(&eng->ev_fork, hipEventDisableTiming) != hipSuccess) return YK_ERR_HIP;
        for (int g = 0; g < G; g++)
            if (hipStreamCreateWithFlags(&eng->gs[g], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&eng->ev_join[g], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&eng->ev_fwd[g], hipEventDisableTiming) != hipSuccess)
                return YK_ERR_HIP;
    }
    if (eng->fparts_dual > 0) {
        if (hipStreamCreateWithFlags(&eng->dstream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&eng->ev_d0, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&eng->ev_d1, hipEventDisableTiming) != hipSuccess)
            return YK_ERR_HIP;
    }
    d.logits = eng->logits;
    d.vpred = eng->vpred;
    d.mlse = eng->mlse;
    d.lut_sq = eng->lut_sq;
    d.lut_sqe = eng->lut_sqe;
    hipLaunchKernelGGL(k_lut, dim3(LUT_N / 256), dim3(256), 0, 0, eng->lut_sq, eng->lut_sqe);
    YK_LAUNCHED();
    YK_HIP(hipMemset(d.err, 0, sizeof(uint32_t)));
    YK_HIP(hipMemset(d.done, 0, E));
    YK_HIP(hipMemset(d.idle, 0, E));
    YK_HIP(hipMemset(d.leaf_state, 0, sizeof(yk_state_t) * E));
    std::vector<uint32_t> ids(E);
    for (size_t i = 0; i < E; i++) ids[i] = (uint32_t)i;
    YK_HIP(hipMemcpy(eng->mcts_env, ids.data(), sizeof(uint32_t) * E, hipMemcpyHostToDevice));
    YK_HIP(hipDeviceSynchronize());
    *out = eng.release();
    return YK_OK;
}

int yk_engine_destroy(yk_engine_t* eng) {
    delete eng;
    return YK_OK;
}

}  // extern "C"

namespace {
// Playout cap: whether move `move` of the batch (seed, env_base) is searched in full.  One
// draw per (batch, move) in its own Philox domain, on the host: no game stream is consumed.
bool playout_full(uint64_t seed, uint32_t env_base, int move, double full_prob) {
    return u53(philox_u64(philox4x32_10(seed, (uint32_t)move, env_base, 0u, PHILOX_PLAYOUT))) < full_prob;
}

// One lock-step batch of complete games: self-play (Coach.executeEpisode) or, with
// d.arena set, Arena.playGame against the uniform-random player.
int play_batch(yk_engine* eng, uint64_t seed, uint32_t env_base, hipStream_t s) {
    EngDev& d = eng->d;
    d.seed = seed;
    const int G = eng->ngroups;
    hipStream_t st[YK_MAX_GROUPS];
    EngDev dg[YK_MAX_GROUPS];
    for (int g = 0; g < G; g++) {
        st[g] = G == 1 ? s : eng->gs[g];
        dg[g] = G == 1 ? d : group_dev(eng, g);
    }
    const dim3 bb(256);
    YK_HIP(hipMemsetAsync(d.err, 0, sizeof(uint32_t), s));
    YK_HIP(hipMemsetAsync(d.hidx[0], 0, sizeof(uint32_t) * (size_t)d.T * d.HCAP, s));
    const bool noise = eng->noise && !d.arena;  // the arenas never add noise
    const bool root_values = eng->root_values && !d.arena;  // nor do they record root values
    const bool capped = eng->fast_sims > 0 && !d.arena;  // nor are they ever capped
    eng->have_priors = false;
    eng->fast_moves = 0;
    // forced playouts and pruning: self-play only, and (below) full moves only - the rule of the root noise
    const bool forcing = eng->forced_k > 0.0 && !d.arena;
    const ForcedDev fd{eng->forced_k, eng->cfg.cpuct};
    if (root_values)  // info[..][7] = 0 also past a game's end: a zero word is "no value recorded"
        YK_HIP(hipMemsetAsync(d.rec_info, 0, sizeof(int32_t) * (size_t)d.E * d.M * 8, s));
    // the self-play temperatures: never in the arenas; the root's where the noise is or would be
    const bool root_temp = eng->root_temp && !d.arena;
    const bool move_temp = eng->move_temp && !d.arena;
    const bool root_edit = noise || root_temp;  // the two launches of k_root_noise per full move
    if (root_edit && eng->nz.prior_after) {  // dense by action: 0 off the valid set and past the game's end
        const size_t nb = sizeof(float) * (((size_t)d.E + d.rec_stride - 1) / d.rec_stride) * (size_t)d.M * ASIZE;
        YK_HIP(hipMemsetAsync(eng->nz.prior_before, 0, nb, s));
        YK_HIP(hipMemsetAsync(eng->nz.prior_after, 0, nb, s));
    }
    YK_HIP(hipMemsetAsync(eng->util_terminals, 0, sizeof(unsigned long long) * (size_t)d.E, s));  // (with the gstats)
    hipLaunchKernelGGL(k_reset, dim3((d.E + 255) / 256), dim3(256), 0, s, d, 1, env_base);
    YK_LAUNCHED();
    if (G > 1) {  // the group streams start after the reset on the caller's stream
        YK_HIP(hipEventRecord(eng->ev_fork, s));
        for (int g = 0; g < G; g++) YK_HIP(hipStreamWaitEvent(st[g], eng->ev_fork, 0));
    }
    eng->have_records = false;
    for (int move = 0; move < d.M; move++) {
        for (int g = 0; g < G; g++) {
            prof_mark(eng, g, KC_MOVE_BEGIN, st[g]);
            hipLaunchKernelGGL(k_move_begin, game_grid(dg[g]), bb, 0, st[g], dg[g], move, 0);
            YK_LAUNCHED();
        }
        // a fast move of the playout cap: fewer simulations, no root noise, the record's status word marked
        const bool fast = capped && !playout_full(seed, env_base, move, eng->full_prob);
        eng->fast_moves += fast;
        if (!d.arena || d.arena_agent == YK_PLAYER_MCTS || d.arena_opp == YK_PLAYER_MCTS) {
            int rc = run_sims(eng, G, st, fast ? eng->fast_sims : d.sims, d.env_id, d.ctr, root_edit && !fast ? move : -1,
                              forcing && !fast ? &fd : nullptr, root_temp ? eng->td.root_t : nullptr, noise);
            if (rc) return rc;
        }
        // the tempered draw: a temp-1 move (k_move_end's own test) whose T is not exactly 1
        const bool temper = move_temp && move + 1 < d.temp_threshold && eng->move_t[move] != 1.0;
        for (int g = 0; g < G; g++) {
            prof_mark(eng, g, KC_MOVE_END, st[g]);
            const bool prune = forcing && !fast && eng->forced_prune;
            yk::with_opts([&](const auto&... o) {  // (prune implies !fast)
                hipLaunchKernelGGL((k_move_end<std::decay_t<decltype(o)>...>), game_grid(dg[g]), bb, 0, st[g], dg[g], move,
                                   fast ? YK_REC_FAST : 0, o...);
            }, yk::opt(prune, fd), yk::opt(temper, eng->td));
            YK_LAUNCHED();
            if (root_values) {  // the games with nmoves == move + 1; root[e] is still this move's root
                prof_mark(eng, g, KC_ROOT_VALUE, st[g]);
                const RootValDev rv{move};
                const int rc = yk_launch_root_value(&dg[g], sizeof(dg[g]), &rv, sizeof(rv), st[g]);
                if (rc) return rc;
            }
            prof_mark(eng, g, -1, st[g]);
            if (G > 1) {
                YK_HIP(hipEventRecord(eng->ev_join[g], st[g]));
                YK_HIP(hipStreamWaitEvent(s, eng->ev_join[g], 0));
            }
        }
        hipLaunchKernelGGL(k_count_done, dim3(1), dim3(1024), 0, s, d.done, d.E, eng->done_count);
        YK_LAUNCHED();
        YK_HIP(hipMemcpyAsync(eng->host_done, eng->done_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        YK_HIP(hipStreamSynchronize(s));
        prof_collect(eng);
        if (*eng->host_done >= d.E) break;
    }
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)(((long)d.E * d.M + 255) / 256)), dim3(256), 0, s, d);
    YK_LAUNCHED();
    eng->have_records = true;
    eng->have_priors = root_edit && eng->nz.prior_after;
    return check_errors(eng, s);
}
}  // namespace

extern "C" {

int yk_selfplay(yk_engine_t* eng, uint64_t seed, uint32_t env_base, void* stream) {
    if (!eng) return YK_ERR_ARG;
    eng->d.arena = 0;
    eng->have_arena = false;
    return play_batch(eng, seed, env_base, as_stream(stream));
}

int yk_engine_set_playout_cap(yk_engine_t* eng, int fast_sims, double full_prob) {
    if (!eng || fast_sims < 0) return YK_ERR_ARG;
    // on: at least 2 simulations (one on a fresh root leaves every visit count zero), at most the full count
    if (fast_sims > 0 && (fast_sims < 2 || fast_sims > eng->d.sims || !(full_prob >= 0.0 && full_prob <= 1.0)))
        return YK_ERR_ARG;
    eng->fast_sims = fast_sims;
    eng->full_prob = full_prob;
    return YK_OK;
}

int yk_engine_set_forced_playouts(yk_engine_t* eng, double k, int prune) {
    if (!eng || !(k >= 0.0) || std::isinf(k) || (prune != 0 && prune != 1)) return YK_ERR_ARG;  // (NaN fails k >= 0)
    eng->forced_k = k;
    eng->forced_prune = prune != 0;
    return YK_OK;
}

int yk_engine_set_fpu(yk_engine_t* eng, int on, double reduction, double root_reduction) {
    if (!eng || !(reduction >= 0.0) || std::isinf(reduction) || !(root_reduction >= 0.0) || std::isinf(root_reduction))
        return YK_ERR_ARG;  // (a NaN fails >= 0)
    eng->fpu_on = on != 0;
    eng->fpu_r = reduction;
    eng->fpu_r_root = root_reduction;
    return YK_OK;
}

int yk_engine_set_score_utility(yk_engine_t* eng, int on, double weight, double scale) {
    if (!eng || !score_knobs_ok(weight, scale)) return YK_ERR_ARG;  // (a NaN fails the comparisons)
    eng->util_on = on != 0;
    eng->util_w = weight;
    eng->util_c = scale;
    return YK_OK;
}

int yk_engine_set_temperatures(yk_engine_t* eng, double move_early, double move_final, double root_early,
                               double root_final, double halflife) {
    if (!eng) return YK_ERR_ARG;
    // a pair of zeros: that schedule is off; else both of its ends within the range (a NaN fails the comparisons)
    const auto pair_ok = [](double a, double b, double lo, double hi) {
        return (a == 0.0 && b == 0.0) || (a >= lo && a <= hi && b >= lo && b <= hi);
    };
    if (!pair_ok(move_early, move_final, 0.05, 100.0) || !pair_ok(root_early, root_final, 0.25, 10.0)) return YK_ERR_ARG;
    if (!(halflife >= 0.0) || std::isinf(halflife)) return YK_ERR_ARG;
    const bool mv = move_final != 0.0, rt = root_final != 0.0;
    if (halflife == 0.0 && ((mv && move_early != move_final) || (rt && root_early != root_final))) return YK_ERR_ARG;
    EngDev& d = eng->d;
    const size_t M = (size_t)d.M, E = (size_t)d.E;
    std::vector<double> mt(M), rtab(M);
    if (mv) YK_TRY(yk_temperature_schedule(move_early, move_final, halflife, d.M, mt.data()));
    if (rt) YK_TRY(yk_temperature_schedule(root_early, root_final, halflife, d.M, rtab.data()));
    YK_HIP(hipDeviceSynchronize());  // (no batch of this engine is in flight while its tables change)
    if (mv) {
        if (!eng->dev_move_t) YK_TRY(eng->mem.alloc(&eng->dev_move_t, M));
        YK_HIP(hipMemcpy(eng->dev_move_t, mt.data(), sizeof(double) * M, hipMemcpyHostToDevice));
    }
    if (rt) {
        if (!eng->dev_root_t) YK_TRY(eng->mem.alloc(&eng->dev_root_t, M));
        YK_HIP(hipMemcpy(eng->dev_root_t, rtab.data(), sizeof(double) * M, hipMemcpyHostToDevice));
        // what the root noise allocates when it is configured: the per-game byte and the prior records
        if (!eng->nz.noised) YK_TRY(eng->mem.alloc(&eng->nz.noised, E));
        if (d.rec_pred && !eng->nz.prior_after) {
            const size_t R = (E + d.rec_stride - 1) / d.rec_stride;
            YK_TRY(eng->mem.alloc(&eng->nz.prior_before, R * M * ASIZE));
            YK_TRY(eng->mem.alloc(&eng->nz.prior_after, R * M * ASIZE));
        }
    }
    eng->move_temp = mv;
    eng->root_temp = rt;
    eng->move_t = mv ? mt : std::vector<double>();
    eng->root_t = rt ? rtab : std::vector<double>();
    eng->td = TemperDev{mv ? eng->dev_move_t : nullptr, rt ? eng->dev_root_t : nullptr};
    return YK_OK;
}

int yk_engine_temperatures(yk_engine_t* eng, double* move_t, double* root_t) {
    if (!eng) return YK_ERR_ARG;
    // HOST [max_moves] each; a schedule that is off reads as zeros
    for (int m = 0; m < eng->d.M; m++) {
        if (move_t) move_t[m] = eng->move_temp ? eng->move_t[m] : 0.0;
        if (root_t) root_t[m] = eng->root_temp ? eng->root_t[m] : 0.0;
    }
    return YK_OK;
}

int yk_playout_schedule(uint64_t seed, uint32_t env_base, double full_prob, int n_moves, uint8_t* full) {
    if (!full || n_moves < 0 || !(full_prob >= 0.0 && full_prob <= 1.0)) return YK_ERR_ARG;
    for (int m = 0; m < n_moves; m++) full[m] = playout_full(seed, env_base, m, full_prob) ? 1 : 0;
    return YK_OK;
}

int yk_arena(yk_engine_t* eng, uint64_t seed, uint32_t env_base, const int32_t* agent_seat, int agent, int opponent,
             void* stream) {
    if (!eng || !agent_seat) return YK_ERR_ARG;
    if (agent < YK_PLAYER_MCTS || agent > YK_PLAYER_GREEDY || opponent < YK_PLAYER_MCTS || opponent > YK_PLAYER_GREEDY)
        return YK_ERR_ARG;
    EngDev& d = eng->d;
    for (int e = 0; e < d.E; e++)
        if (agent_seat[e] != 1 && agent_seat[e] != -1) return YK_ERR_ARG;
    hipStream_t s = as_stream(stream);
    YK_HIP(hipMemcpyAsync(d.seat, agent_seat, sizeof(int32_t) * (size_t)d.E, hipMemcpyHostToDevice, s));
    d.arena = 1;
    d.arena_agent = agent;
    d.arena_opp = opponent;
    // two MCTS players each keep their own tree (and net) when the engine has dual trees
    d.dual = (d.T == 2 * d.E && agent == YK_PLAYER_MCTS && opponent == YK_PLAYER_MCTS) ? 1 : 0;
    if (d.dual && eng->dstream) d.fparts = eng->fparts_dual;  // the two seats' forwards side by side
    eng->have_arena = false;
    const int rc = play_batch(eng, seed, env_base, s);
    d.arena = 0;
    d.dual = 0;
    d.fparts = eng->fparts_single;
    eng->have_arena = rc == YK_OK || rc == YK_ERR_STATE;
    return rc;
}

int yk_engine_set_opponent_net(yk_engine_t* eng, yk_net_t* net) {
    if (!eng || !net) return YK_ERR_ARG;
    if (eng->d.T != 2 * eng->d.E || eng->d.prior != 0) return YK_ERR_ARG;  // needs dual trees and the net prior
    if (net->dev.H != eng->net->dev.H) return YK_ERR_ARG;
    eng->net2 = net;
    return YK_OK;
}

int yk_arena_results(yk_engine_t* eng, double* result, int32_t* totals, int32_t* n_moves, int32_t* actions,
                     uint64_t* final_states, uint64_t* rng_ctr) {
    if (!eng) return YK_ERR_ARG;
    if (!eng->have_arena) return YK_ERR_STATE;
    EngDev& d = eng->d;
    const size_t E = d.E, M = d.M;
    YK_HIP(hipDeviceSynchronize());
    std::vector<int32_t> nm(E), fc(E), info;
    std::vector<double> fr(E);
    YK_HIP(hipMemcpy(nm.data(), d.nmoves, sizeof(int32_t) * E, hipMemcpyDeviceToHost));
    if (result) {
        YK_HIP(hipMemcpy(fr.data(), d.final_r, sizeof(double) * E, hipMemcpyDeviceToHost));
        YK_HIP(hipMemcpy(fc.data(), d.final_cur, sizeof(int32_t) * E, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < E; e++) result[e] = (double)fc[e] * fr[e];  // Arena.py:93
    }
    if (totals) YK_HIP(hipMemcpy(totals, d.final_tot, sizeof(int32_t) * 2 * E, hipMemcpyDeviceToHost));
    if (n_moves) std::copy(nm.begin(), nm.end(), n_moves);
    if (actions) {
        info.resize(E * M * 8);
        YK_HIP(hipMemcpy(info.data(), d.rec_info, sizeof(int32_t) * info.size(), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < E; e++)
            for (size_t m = 0; m < M; m++) actions[e * M + m] = (int)m < nm[e] ? info[(e * M + m) * 8 + 2] : -1;
    }
    if (final_states) YK_HIP(hipMemcpy(final_states, d.board, sizeof(yk_state_t) * E, hipMemcpyDeviceToHost));
    if (rng_ctr) YK_HIP(hipMemcpy(rng_ctr, d.ctr, sizeof(uint64_t) * E, hipMemcpyDeviceToHost));
    return YK_OK;
}

int yk_engine_profile(yk_engine_t* eng, int enable) {
    if (!eng) return YK_ERR_ARG;
    if (enable < 0) return YK_ERR_ARG;
    eng->prof = enable != 0;
    eng->prof_stride = enable > 0 ? enable : 1;
    for (auto& L : eng->pg) L.used = 0;
    for (int i = 0; i < 8; i++) {
        eng->kms[i] = 0;
        eng->klaunch[i] = 0;
    }
    return YK_OK;
}

int yk_engine_kernel_times(yk_engine_t* eng, double* ms, int64_t* launches) {
    if (!eng || !ms || !launches) return YK_ERR_ARG;
    for (int i = 0; i < 8; i++) {
        ms[i] = eng->kms[i];
        launches[i] = eng->klaunch[i];
    }
    return YK_OK;
}

int yk_engine_stats(yk_engine_t* eng, int64_t* out) {
    if (!eng || !out) return YK_ERR_ARG;
    EngDev& d = eng->d;
    std::vector<uint64_t> gs((size_t)d.E * GST);
    std::vector<int32_t> nm(d.E);
    uint32_t err = 0;
    YK_HIP(hipDeviceSynchronize());
    YK_HIP(hipMemcpy(gs.data(), d.gstats, sizeof(uint64_t) * gs.size(), hipMemcpyDeviceToHost));
    YK_HIP(hipMemcpy(nm.data(), d.nmoves, sizeof(int32_t) * nm.size(), hipMemcpyDeviceToHost));
    YK_HIP(hipMemcpy(&err, d.err, sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < 16; i++) out[i] = 0;
    for (int e = 0; e < d.E; e++) {
        const uint64_t* g = &gs[(size_t)e * GST];
        out[0] += (int64_t)g[0];
        out[1] += (int64_t)g[1];
        out[2] = std::max<int64_t>(out[2], nm[e]);
        out[4] = std::max<int64_t>(out[4], (int64_t)g[4]);
        out[5] = std::max<int64_t>(out[5], (int64_t)g[5]);
        out[6] = std::max<int64_t>(out[6], (int64_t)g[6]);
        out[7] += (int64_t)g[3];
        out[8] += (int64_t)g[2];
        out[9] = std::max<int64_t>(out[9], (int64_t)g[7]);
    }
    out[3] = err;
    out[10] = d.NCAP;
    out[11] = d.ECAP;
    out[12] = d.AE;
    out[13] = d.VCAP;
    out[14] = eng->ngroups;
    out[15] = d.fparts;
    return YK_OK;
}

int yk_engine_counters(yk_engine_t* eng, int64_t* out, int n) {
    if (!eng || !out || n < 0) return YK_ERR_ARG;
    EngDev& d = eng->d;
    std::vector<uint64_t> gs((size_t)d.E * GST);
    YK_HIP(hipDeviceSynchronize());
    YK_HIP(hipMemcpy(gs.data(), d.gstats, sizeof(uint64_t) * gs.size(), hipMemcpyDeviceToHost));
    // scan edges; expansions by prior path: window, sparse, general; the playout cap's fast moves; root picks
    // that took a forced edge and visits the pruning took off the recorded counts; descent picks
    // first-play urgency gave to the unvisited candidate, and picks its rule decided; descents
    // that ended at a terminal state and returned a score-margin utility
    std::vector<unsigned long long> ut((size_t)d.E);
    YK_HIP(hipMemcpy(ut.data(), eng->util_terminals, sizeof(unsigned long long) * ut.size(), hipMemcpyDeviceToHost));
    int64_t c[10] = {0, 0, 0, 0, eng->fast_moves, 0, 0, 0, 0, 0};
    for (int e = 0; e < d.E; e++) {
        c[0] += (int64_t)gs[(size_t)e * GST + 8];
        for (int k = 0; k < 3; k++) c[1 + k] += (int64_t)gs[(size_t)e * GST + 9 + k];
        for (int k = 0; k < 4; k++) c[5 + k] += (int64_t)gs[(size_t)e * GST + 12 + k];
        c[9] += (int64_t)ut[e];
    }
    for (int i = 0; i < n; i++) out[i] = i < 10 ? c[i] : 0;
    return YK_OK;
}

int yk_engine_records(yk_engine_t* eng, uint64_t* states, int32_t* info, uint64_t* ctr, double* values,
                      uint64_t* final_states, int32_t* n_moves, int64_t* visits_off, int32_t* visits,
                      int64_t* n_visits) {
    if (!eng) return YK_ERR_ARG;
    if (!eng->have_records) return YK_ERR_STATE;
    EngDev& d = eng->d;
    const size_t E = d.E, M = d.M;
    YK_HIP(hipDeviceSynchronize());
    if (states) YK_HIP(hipMemcpy(states, d.rec_state, sizeof(yk_state_t) * E * M, hipMemcpyDeviceToHost));
    if (info) YK_HIP(hipMemcpy(info, d.rec_info, sizeof(int32_t) * E * M * 8, hipMemcpyDeviceToHost));
    if (ctr) YK_HIP(hipMemcpy(ctr, d.rec_ctr, sizeof(uint64_t) * E * M * 2, hipMemcpyDeviceToHost));
    if (values) YK_HIP(hipMemcpy(values, d.rec_val, sizeof(double) * E * M, hipMemcpyDeviceToHost));
    if (final_states) YK_HIP(hipMemcpy(final_states, d.board, sizeof(yk_state_t) * E, hipMemcpyDeviceToHost));
    if (n_moves) YK_HIP(hipMemcpy(n_moves, d.nmoves, sizeof(int32_t) * E, hipMemcpyDeviceToHost));
    if (visits_off || visits || n_visits) {
        std::vector<int32_t> voff(E * (M + 1));
        std::vector<int32_t> nm(E);
        YK_HIP(hipMemcpy(voff.data(), d.rec_voff, sizeof(int32_t) * voff.size(), hipMemcpyDeviceToHost));
        YK_HIP(hipMemcpy(nm.data(), d.nmoves, sizeof(int32_t) * E, hipMemcpyDeviceToHost));
        int64_t total = 0;
        for (size_t e = 0; e < E; e++) total += voff[e * (M + 1) + nm[e]];
        if (n_visits) *n_visits = total;
        if (visits_off || visits) {
            std::vector<uint32_t> raw(E * (size_t)d.VCAP);
            YK_HIP(hipMemcpy(raw.data(), d.rec_visits, sizeof(uint32_t) * raw.size(), hipMemcpyDeviceToHost));
            int64_t k = 0;
            for (size_t e = 0; e < E; e++) {
                for (size_t m = 0; m < M; m++) {
                    const int32_t a0 = voff[e * (M + 1) + m];
                    const int32_t a1 = (int)m < nm[e] ? voff[e * (M + 1) + m + 1] : a0;
                    if (visits_off) visits_off[e * M + m] = k;
                    for (int32_t i = a0; i < a1; i++, k++)
                        if (visits) {
                            const uint32_t x = raw[e * d.VCAP + i];
                            visits[2 * k] = (int32_t)(x >> 16);
                            visits[2 * k + 1] = (int32_t)(x & 0xFFFF);
                        }
                }
            }
            if (visits_off) visits_off[E * M] = k;
        }
    }
    return YK_OK;
}

int yk_engine_predictions(yk_engine_t* eng, float* pi, float* v, yk_state_t* leaves, int32_t* count) {
    if (!eng || !eng->d.rec_pred) return YK_ERR_ARG;
    EngDev& d = eng->d;
    const size_t R = ((size_t)d.E + d.rec_stride - 1) / d.rec_stride, X = (size_t)d.max_exp;
    YK_HIP(hipDeviceSynchronize());
    if (pi) YK_HIP(hipMemcpy(pi, d.rec_pi, sizeof(float) * R * X * ASIZE, hipMemcpyDeviceToHost));
    if (v) YK_HIP(hipMemcpy(v, d.rec_v, sizeof(float) * R * X, hipMemcpyDeviceToHost));
    if (leaves) YK_HIP(hipMemcpy(leaves, d.rec_leaf, sizeof(yk_state_t) * R * X, hipMemcpyDeviceToHost));
    if (count) {
        std::vector<uint64_t> gs((size_t)d.E * GST);
        YK_HIP(hipMemcpy(gs.data(), d.gstats, sizeof(uint64_t) * gs.size(), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < R; r++) count[r] = (int32_t)gs[r * d.rec_stride * GST];  // > max_expansions: truncated
    }
    return YK_OK;
}

int yk_engine_root_priors(yk_engine_t* eng, float* before, float* after) {
    if (!eng) return YK_ERR_ARG;
    if (!eng->have_priors) return YK_ERR_STATE;
    EngDev& d = eng->d;
    const size_t n = (((size_t)d.E + d.rec_stride - 1) / d.rec_stride) * (size_t)d.M * ASIZE;
    YK_HIP(hipDeviceSynchronize());
    if (before) YK_HIP(hipMemcpy(before, eng->nz.prior_before, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (after) YK_HIP(hipMemcpy(after, eng->nz.prior_after, sizeof(float) * n, hipMemcpyDeviceToHost));
    return YK_OK;
}

int yk_engine_root_prior(yk_engine_t* eng, int game, float* p) {
    if (!eng || !p || game < 0 || game >= eng->d.E) return YK_ERR_ARG;
    EngDev& d = eng->d;
    uint4 rc[2];
    YK_HIP(hipDeviceSynchronize());
    YK_HIP(hipMemcpy(rc, d.root_c + 2 * game, sizeof(rc), hipMemcpyDeviceToHost));
    if (rc[0].x == 0) return YK_ERR_STATE;  // no descent of the move found the root in the tree
    const uint64_t x = (uint64_t)rc[1].x | ((uint64_t)rc[1].y << 32);  // (pack_vinfo)
    VInfo vi;
    vi.cats = x & 0xFFFFFFFFFFFFull;
    vi.k = (int)((x >> 48) & 0xF);
    vi.n = (int)((x >> 52) & 0xF);
    vi.W = (int)(x >> 56);
    vi.V = (int)rc[0].z;
    std::vector<float> P((size_t)vi.V);
    if (vi.V > 0)
        YK_HIP(hipMemcpy(P.data(), d.arenaP + (size_t)game * d.AE + rc[0].y, sizeof(float) * P.size(), hipMemcpyDeviceToHost));
    for (int a = 0; a < ASIZE; a++) p[a] = 0.f;
    for (int j = 0; j < vi.V; j++) p[compact_to_action(vi, j)] = P[j];
    return YK_OK;
}

static void record_parts(yk_engine* eng, void** p, RecordLayout& L) {
    EngDev& d = eng->d;
    L = record_layout(d.E, d.M, d.VCAP);
    void* pp[REC_PARTS] = {d.rec_state, d.rec_info, d.rec_ctr, d.rec_val, d.rec_visits, d.rec_voff, d.nmoves, d.board};
    for (int i = 0; i < REC_PARTS; i++) p[i] = pp[i];
}

int64_t yk_engine_record_bytes(yk_engine_t* eng) {
    if (!eng) return YK_ERR_ARG;
    return record_layout(eng->d.E, eng->d.M, eng->d.VCAP).total;
}

int yk_engine_pack_records(yk_engine_t* eng, void* dst, int64_t capacity, void* stream) {
    if (!eng || !dst) return YK_ERR_ARG;
    if (!eng->have_records) return YK_ERR_STATE;
    void* p[REC_PARTS];
    RecordLayout L;
    record_parts(eng, p, L);
    if (capacity < L.total) return YK_ERR_ARG;
    for (int i = 0; i < REC_PARTS; i++)
        YK_HIP(hipMemcpyAsync((char*)dst + L.off[i], p[i], (size_t)L.bytes[i], hipMemcpyDeviceToDevice,
                              as_stream(stream)));
    return YK_OK;
}

int yk_mcts_reset(yk_engine_t* eng) {
    if (!eng) return YK_ERR_ARG;
    EngDev& d = eng->d;
    YK_HIP(hipMemset(d.err, 0, sizeof(uint32_t)));
    YK_HIP(hipMemset(d.hidx[0], 0, sizeof(uint32_t) * (size_t)d.T * d.HCAP));
    YK_HIP(hipMemset(d.done, 0, (size_t)d.E));
    YK_HIP(hipMemset(eng->util_terminals, 0, sizeof(unsigned long long) * (size_t)d.E));  // (with the gstats)
    hipLaunchKernelGGL(k_reset, dim3((d.E + 255) / 256), dim3(256), 0, 0, d, 0, 0u);
    YK_LAUNCHED();
    YK_HIP(hipDeviceSynchronize());
    return YK_OK;
}

int yk_mcts_search(yk_engine_t* eng, const yk_state_t* roots, uint64_t seed, const uint32_t* env_ids,
                   uint64_t* rng_ctr, int sims, int32_t* counts, void* stream) {
    if (!eng || !roots || !env_ids || !rng_ctr || !counts || sims < 0) return YK_ERR_ARG;
    hipStream_t s = as_stream(stream);
    EngDev& d = eng->d;
    d.seed = seed;
    const dim3 gb = game_grid(d), bb(256);
    YK_HIP(hipMemcpyAsync(d.root, roots, sizeof(yk_state_t) * (size_t)d.E, hipMemcpyDeviceToDevice, s));
    YK_HIP(hipMemsetAsync(d.done, 0, (size_t)d.E, s));
    YK_HIP(hipMemsetAsync(d.err, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_move_begin, gb, bb, 0, s, d, 0, 1);
    YK_LAUNCHED();
    int rc = run_sims(eng, 1, &s, sims, env_ids, rng_ctr);  // the plugin path: one group on the caller's stream
    if (rc) return rc;
    hipLaunchKernelGGL(k_root_counts, gb, bb, 0, s, d, counts);
    YK_LAUNCHED();
    return check_errors(eng, s);
}

}  // extern "C"
