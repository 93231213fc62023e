// yk_noise.hip - Dirichlet root noise of self-play: the kernel that mixes eta ~ Dir(alpha)
// into each real move's root prior, and the standalone sampler entry point.  Both run block_dirichlet
// (yk_noise.h), so the noise a search sees and the noise yk_dirichlet_noise returns are the same bits.
// The same kernel, as a template, also applies the root policy temperature (yk_temper.h): the
// root's prior is edited in one place, at most once per move.
#include <string.h>

#include "yk_engine_dev.h"
#include "yk_noise.h"
#include "yk_optarg.h"
#include "yk_temper.h"

namespace {

// Dirichlet root noise: once per real move of a self-play game the root's stored prior
// becomes P'[j] = f32((1 - eps) (f64)P[j] + eps eta[j]), eta ~ Dir(alpha) over its compact valid set
// (block_dirichlet, yk_noise.h).  In place: the game only moves forward, so a past root is never
// reached again and no other node's scan sees the change.  One workgroup per game, two phases (the
// top of getActionProb, MCTS.py:37):
//   phase 0, before the move's first descent: a root already in the tree is noised and the game's
//            byte set; the byte is cleared when the root is not expanded yet;
//   phase 1, after simulation 0's expansion (which, with the byte clear, only expanded the root and
//            returned, MCTS.py:84-115): the games whose byte is clear.
// A root with Ns = 0 has had no scan yet: its summary first_j is recomputed from P' with the scan's
// own f32 operations (the expansion's, lowest index among equals).  k_root_sort runs after phase 1,
// so the root's order is P''s.
// TEMPER (the root policy temperature; the table of T by move in the pack, yk_optarg.h): P is first
// replaced by f32(P^(1/T) / S) over the same compact set (block_temper_weights, yk_temper.h: P read from
// memory once, the weights staged in LDS), and the noise then mixes from that rounded value - one launch
// does both.  NOISE = false is the tempering alone, without the sampler.  T == 1.0 exactly, or a prior
// whose weights do not sum to > 0, leaves P as it is.  <true>, the empty pack, is the kernel the noise alone runs.
template <bool NOISE, class... TD>
__global__ __launch_bounds__(NOISE_THREADS) void k_root_noise(EngDev d, NoiseDev nz, int move, int phase, TD... root_t) {
    constexpr bool TEMPER = yk::has_arg<const double*, TD...>;
    static_assert(yk::args_in(yk::Args<const double*>{}, yk::Args<TD...>{}) && (TEMPER || NOISE), "the table of T or nothing");
    static_assert(TEMPER_THREADS == NOISE_THREADS, "one workgroup shape");
    __shared__ double eta[NOISE ? ASIZE : 1];
    __shared__ double wsum[4];
    __shared__ double tw[TEMPER ? ASIZE : 1];
    __shared__ double tsum[4];
    __shared__ int s_nid;
    __shared__ float s_fb[NOISE_THREADS / 64];
    __shared__ int s_fj[NOISE_THREADS / 64];
    const int e = d.e_lo + (int)blockIdx.x;
    if (e >= d.e_hi || d.done[e] || d.idle[e]) return;
    if (phase == 1 && nz.noised[e]) return;
    const int tid = threadIdx.x;
    const int t = tree_of(d, e);
    const int g = d.gen[t];
    if (tid < 64) {
        const YkS r = ld_state(d.root + e);
        const int nid = lookup(d, g, t, r, index_hash(r));
        if (tid == 0) s_nid = nid;
    }
    __syncthreads();  // (every thread has read the byte by now)
    const int nid = s_nid;
    if (tid == 0) nz.noised[e] = nid >= 0 ? 1 : 0;
    if (nid < 0) return;  // phase 1: simulation 0 could not expand the root (k_move_end reports it)
    NodeRec& nd = d.nodes[g][(long)t * d.NCAP + nid];
    const int V = (int)nd.nvalid;
    if (V <= 0 || V > ASIZE) return;
    const uint32_t Ns = nd.Ns;
    float* P = d.arenaP + (long)t * d.AE + nd.p_off;
    if constexpr (NOISE) block_dirichlet(d.seed, d.env_id[e], (uint32_t)move, V, nz.alpha, eta, wsum);
    const bool rec = nz.prior_after && d.rec_pred && (e % d.rec_stride) == 0 && move < d.M;
    const long rslot = rec ? ((long)(e / d.rec_stride) * d.M + move) * ASIZE : 0;
    const VInfo vi = unpack_vinfo(nd.vinfo, (uint32_t)V);
    const double keep = 1.0 - nz.eps;
    const float sqe0 = (float)sqrt((double)0u + 1e-8);
    bool tempered = false;  // (block-uniform)
    double S = 0.0;
    if constexpr (TEMPER) {
        const double T = yk::get_arg<const double*>(root_t...)[move];
        if (T != 1.0) {
            S = block_temper_weights(P, V, 1.0 / T, tw, tsum, [&](int j, float p) {
                if (rec) nz.prior_before[rslot + compact_to_action(vi, j)] = p;
            });
            tempered = S > 0.0;
        }
    }
    float fb = -INFINITY;
    int fj = 0x7FFFFFFF;
    for (int j = tid; j < V; j += NOISE_THREADS) {
        const float p = (TEMPER && tempered) ? tempered_prior(tw[j], S) : P[j];
        float q = p;
        if constexpr (NOISE) q = (float)(keep * (double)p + nz.eps * eta[j]);
        if (NOISE || tempered) P[j] = q;
        if (rec) {
            const int a = compact_to_action(vi, j);
            if (!(TEMPER && tempered)) nz.prior_before[rslot + a] = p;  // (tempered: the first pass recorded it)
            nz.prior_after[rslot + a] = q;
        }
        const float u0 = (d.c32 * q) * sqe0;
        if (u0 > fb) {  // ascending j within the thread: strict '>' keeps the lowest
            fb = u0;
            fj = j;
        }
    }
    if (Ns != 0) return;  // (block-uniform) the node's first scan is behind it: the summary is not read again
    wave_argmax_step(fb, fj);
    if ((tid & 63) == 0) {
        s_fb[tid >> 6] = fb;
        s_fj[tid >> 6] = fj;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NOISE_THREADS / 64; w++)
            if (s_fb[w] > fb || (s_fb[w] == fb && s_fj[w] < fj)) {
                fb = s_fb[w];
                fj = s_fj[w];
            }
        nd.first_j = (uint32_t)fj;
    }
}

// yk_dirichlet_noise: row i's eta for (seed, env_ids[i], moves[i], nvalid[i], alpha) - the engine's
// block_dirichlet - dense over 3226 columns, 0 past nvalid[i].  One workgroup per row.
__global__ __launch_bounds__(NOISE_THREADS) void k_dirichlet_rows(uint64_t seed, const uint32_t* env_ids,
                                                                  const int32_t* moves, const int32_t* nvalid,
                                                                  double alpha, double* out, int n) {
    __shared__ double eta[ASIZE];
    __shared__ double wsum[4];
    const int i = (int)blockIdx.x;
    if (i >= n) return;
    const int V = min(max(nvalid[i], 0), ASIZE);
    if (V > 0) block_dirichlet(seed, env_ids[i], (uint32_t)moves[i], V, alpha, eta, wsum);
    double* o = out + (long)i * ASIZE;
    for (int j = threadIdx.x; j < ASIZE; j += NOISE_THREADS) o[j] = j < V ? eta[j] : 0.0;
}

}  // namespace

int yk_launch_root_noise(const void* engdev, size_t engdev_bytes, const void* noisedev, size_t noisedev_bytes, int move,
                         int phase, hipStream_t stream) {
    if (!engdev || !noisedev || engdev_bytes != sizeof(EngDev) || noisedev_bytes != sizeof(NoiseDev)) return YK_ERR_ARG;
    EngDev d;
    NoiseDev nz;
    memcpy(&d, engdev, sizeof(d));
    memcpy(&nz, noisedev, sizeof(nz));
    if (d.e_hi <= d.e_lo) return YK_OK;
    hipLaunchKernelGGL((k_root_noise<true>), dim3((unsigned)(d.e_hi - d.e_lo)), dim3(NOISE_THREADS), 0, stream, d,
                       nz, move, phase);
    YK_LAUNCHED();
    return YK_OK;
}

int yk_launch_root_temper(const void* engdev, size_t engdev_bytes, const void* noisedev, size_t noisedev_bytes,
                          const double* root_t, int with_noise, int move, int phase, hipStream_t stream) {
    if (!engdev || !noisedev || !root_t || engdev_bytes != sizeof(EngDev) || noisedev_bytes != sizeof(NoiseDev))
        return YK_ERR_ARG;
    EngDev d;
    NoiseDev nz;
    memcpy(&d, engdev, sizeof(d));
    memcpy(&nz, noisedev, sizeof(nz));
    if (move < 0 || move >= d.M) return YK_ERR_ARG;  // the table has M entries
    if (d.e_hi <= d.e_lo) return YK_OK;
    const dim3 grid((unsigned)(d.e_hi - d.e_lo)), block(NOISE_THREADS);
    if (with_noise)
        hipLaunchKernelGGL((k_root_noise<true, const double*>), grid, block, 0, stream, d, nz, move, phase, root_t);
    else
        hipLaunchKernelGGL((k_root_noise<false, const double*>), grid, block, 0, stream, d, nz, move, phase, root_t);
    YK_LAUNCHED();
    return YK_OK;
}

extern "C" int yk_dirichlet_noise(uint64_t seed, const uint32_t* env_ids, const int32_t* moves, const int32_t* nvalid,
                                  double alpha, double* eta, int n, void* stream) {
    if (!env_ids || !moves || !nvalid || !eta || n < 0 || !(alpha > 0.0)) return YK_ERR_ARG;
    if (n == 0) return YK_OK;
    hipLaunchKernelGGL(k_dirichlet_rows, dim3((unsigned)n), dim3(NOISE_THREADS), 0, as_stream(stream), seed, env_ids,
                       moves, nvalid, alpha, eta, n);
    YK_LAUNCHED();
    return YK_OK;
}
