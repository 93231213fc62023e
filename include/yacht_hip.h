/*
 * yacht_hip.h - C ABI of libyacht_hip.so, the MI355X (gfx950) self-play engine for
 * Yacht Auction.  This is the drop-in boundary for the reference's hot path
 *   Coach.executeEpisode -> MCTS.getActionProb -> MCTS.search
 *     -> YachtGame.{getNextState,getValidMoves,getGameEnded,getCanonicalForm,...}
 *     -> NNetWrapper.predict
 * (paths relative to the reference repository iyioon/NYPC-Yacht-Auction).
 *
 * Conventions
 *  - Every array argument is a DEVICE pointer owned by the caller (hipMalloc /
 *    torch), unless the comment says "host".  `stream` is a hipStream_t (NULL = the
 *    default stream).  Calls are asynchronous on `stream` unless they say otherwise.
 *  - Return value: YK_OK (0) or a negative YK_ERR_* code (API / HIP / capacity error).
 *    The reference's per-call Python exceptions are reported per element in a
 *    `status` array (YK_ST_*), because a batch can contain both good and bad inputs.
 *  - A game state is the 64-byte packed yk_state_t (layout: DESIGN.md section 3; it is
 *    injective on exactly the fields of YachtGame.stringRepresentation, so two states
 *    are the same MCTS node iff their 8 words are equal).
 *  - Randomness: the reference draws from process-global numpy / `random` RNGs
 *    (YachtGame.py:154-159, MCTS.py:46, Coach.py:65).  Here every game owns a stream
 *    (seed, env_id, counter) of Philox4x32-10 draws; each die, tie-break, tie pick and
 *    sampling uniform consumes one counter value.  Given the same draws the results
 *    are identical to the reference (tests/test_oracle_golden.py, tests/test_gpu_*.py).
 *    Counter word 3 is the domain of a draw (0 for the game streams); the domains the
 *    entry points below name are listed once, in csrc/yk_philox.h.
 *  - No torch types cross this boundary.
 */
#ifndef YACHT_HIP_H
#define YACHT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YK_ACTION_SIZE 3226   /* YachtGame.py:42 */
#define YK_NUM_BID_ACTIONS 202 /* YachtGame.py:32 */
#define YK_FEATURES 59        /* YachtGame.getBoardSize, NNet.py:47 */
#define YK_MASK_WORDS 101     /* ceil(3226 / 32) */

typedef struct { uint64_t w[8]; } yk_state_t;

/* return codes */
#define YK_OK 0
#define YK_ERR_ARG (-1)
#define YK_ERR_HIP (-2)
#define YK_ERR_NOMEM (-3)
#define YK_ERR_CAPACITY (-4) /* a fixed-size engine pool overflowed; results invalid */
#define YK_ERR_STATE (-5)    /* engine misuse (e.g. MCTS root round went backwards) */
#define YK_ERR_RANGE (-6)    /* a value outside the range an operation accepts: a net weight outside the fp16
                                split's (|w| >= 65520: its hi plane overflows); a sampling weight that is negative
                                or NaN, or weights whose total is not finite and > 0 (yk_sample_cdf); row indices not
                                strictly ascending within a CSR (yk_policies_splice) or outside it (yk_policies_take) */

/* per-element status of yk_step: the reference's exceptions */
#define YK_ST_OK 0
#define YK_ST_VALUE_BID 1   /* ValueError("Invalid action in BID phase")   YachtGame.py:268-269 */
#define YK_ST_VALUE_SCORE 2 /* ValueError("Invalid action in SCORE phase") YachtGame.py:306-307 */
#define YK_ST_RUNTIME 3     /* RuntimeError("Invalid phase/state")          YachtGame.py:372 */
#define YK_ST_ASSERT 4      /* AssertionError, _resolve_bids_and_assign     YachtGame.py:508 */
#define YK_ST_CAPACITY 5    /* a carry would exceed 10 dice (unreachable from getInitBoard) */

const char* yk_version(void);
/* last HIP error code seen by the library (hipError_t as int), 0 if none */
int yk_last_hip_error(void);
/* HOST: draw `ctr` of game `env`'s stream (Philox4x32-10, key = seed, counter = (ctr, env, 0)):
 * low 32 bits = word 0, high = word 1.  die = 1 + ((d >> 32) * 6 >> 32), below(n) likewise,
 * uniform = (d >> 11) * 2^-53. */
uint64_t yk_rng_draw64(uint64_t seed, uint32_t env, uint64_t ctr);

/* ---------------------------------------------------------------- Game plugin (batched)
 * Replaces YachtGame (yacht/YachtGame.py:210-467) behind Game.py:14-113.  Player values
 * follow the reference: 1 = player 1, anything else = player 2 (-1). */

/* getInitBoard (YachtGame.py:232-237): draws rollA then rollB (10 dice) from each game's
 * stream; rng_ctr[i] is read and advanced. */
int yk_init_board(yk_state_t* out, uint64_t* rng_ctr, const uint32_t* env_ids, uint64_t seed, int n,
                  void* stream);
/* getNextState (YachtGame.py:260-372, _resolve_bids_and_assign :502-542).  Pure: `in` is
 * not modified (out may alias in).  rng_ctr advanced by the draws made (tie-break, re-rolls).
 * status[i] != YK_ST_OK => out[i] / next_players[i] / rng_ctr[i] unspecified (the
 * reference raised).  The silent no-op of an illegal SCORE action is YK_ST_OK with the
 * state copied and the player flipped (YachtGame.py:312-314, 322-324). */
int yk_step(const yk_state_t* in, const int32_t* players, const int32_t* actions, uint64_t seed,
            const uint32_t* env_ids, uint64_t* rng_ctr, yk_state_t* out, int32_t* next_players, int8_t* status,
            int n, void* stream);
/* getValidMoves (YachtGame.py:374-406) as a bitmask: bit (a & 31) of mask[i*101 + a/32];
 * counts[i] = number of valid actions (may be NULL). */
int yk_valid_mask(const yk_state_t* in, const int32_t* players, uint32_t* mask, int32_t* counts, int n,
                  void* stream);
/* getGameEnded (YachtGame.py:408-428): result[i] in {0, 1e-4, 1, -1} (python float);
 * totals[i*2+{0,1}] = total_with_bonus of p1/p2 (YachtGame.py:128-130), may be NULL. */
int yk_ended(const yk_state_t* in, const int32_t* players, double* result, int32_t* totals, int n, void* stream);
/* getCanonicalForm (YachtGame.py:430-442): player 1 -> copy; else p1<->p2 and bids swapped
 * (the reference does NOT mask the pending bid, despite its docstring). */
int yk_canonical(const yk_state_t* in, const int32_t* players, yk_state_t* out, int n, void* stream);
/* score_category (YachtGame.py:57-108) of every (category, combo) on the mover's carry:
 * out[(i*12 + cat)*252 + combo]; -1 where combo position >= len(carry). */
int yk_score_table(const yk_state_t* in, const int32_t* players, int32_t* out, int n, void* stream);
/* score_category on explicit dice: dice[i*5..+5] in 1..6 -> out[i*12 + cat]. */
int yk_score_dice(const int8_t* dice, int32_t* out, int n, void* stream);
/* state_to_vec (yacht/NNet.py:65-86), bit-exact float32: x[i*59 + f]. */
int yk_featurize(const yk_state_t* in, float* x, int n, void* stream);
/* 64-bit transposition-key hash (stands in for stringRepresentation, YachtGame.py:448-467). */
int yk_key_hash(const yk_state_t* in, uint64_t* out, int n, void* stream);
/* GreedyYachtPlayer's heuristic (yacht/YachtPlayers.py:38-171) on canonical boards (device):
 * actions[i] = the heuristic's action, or -1 when it is not a valid move (the player then
 * plays np.random.choice(legal), YachtPlayers.py:199-214). */
int yk_greedy_action(const yk_state_t* states, int32_t* actions, int n, void* stream);
/* Deterministic test prior (oracle/spec.py hash_prior): pi[i*3226 + a], v[i]. */
int yk_hash_prior(const yk_state_t* in, float* pi, float* v, int n, void* stream);

/* ---------------------------------------------------------------- NeuralNet.predict
 * Replaces NNetWrapper.predict (yacht/NNet.py:177-195) over YachtNNet
 * (yacht/pytorch/YachtNNet.py:8-70), eval mode, batched, float32 (MFMA f32). */
typedef struct yk_net yk_net_t;
/* params: HOST float32 arrays in YachtNNet.state_dict() order (inp.0.weight, inp.0.bias,
 * inp.1.weight, inp.1.bias, blocks.{b}.{fc1,ln1,fc2,ln2}.{weight,bias}, pi_head.0.*,
 * pi_head.2.*, v_head.0.*, v_head.2.*, v_head.4.*).  hidden in {64,128,256,512}, nblocks 0-64.
 * YK_ERR_RANGE when a finite weight of a Linear layer overflows the fp16 hi plane of the
 * f32-equivalent split (|w| >= 65520): the planes would hold inf where torch holds a number. */
int yk_net_create(yk_net_t** net, int hidden, int nblocks, const float* const* params, int nparams);
/* pi[i*3226 + a] = exp(log_softmax(logits)), v[i] = tanh(v_head). */
int yk_net_predict(yk_net_t* net, const yk_state_t* states, float* pi, float* v, int n, void* stream);
/* same from explicit feature rows x[i*59 + f] */
int yk_net_predict_features(yk_net_t* net, const float* x, float* pi, float* v, int n, void* stream);
/* The prior the self-play engine expands a leaf with (MCTS.py:86-88 inside yk_selfplay), before
 * its renormalisation: pi[i*3226 + a] = exp(x_a - m - l) at the valid actions of canonical state
 * i (getValidMoves(s, 1)), 0 elsewhere, with (m, l) the softmax statistics over the actions of the
 * 16-action tiles holding those valid actions - or over all 3226 logits (NNetWrapper.predict's pi,
 * masked) when a weight-norm bound cannot rule out that every valid pi underflows in the full
 * softmax.  Renormalised over the valid actions it is MCTS.py:88-91's P either way. */
int yk_net_leaf_prior(yk_net_t* net, const yk_state_t* states, float* pi, float* v, int n, void* stream);
/* The submission bot's move (replaces AIPlayer.get_move's network part,
 * yacht/submission/agent.py:248-280): for canonical states (the mover is p1), the action of
 * highest softmax probability among the decodable ones (agent.py:150-187, the same set as
 * getValidMoves), lowest index on equal probability; -1 when none.  probs (optional) gets
 * that probability.  Device pointers. */
int yk_net_policy_action(yk_net_t* net, const yk_state_t* states, int32_t* actions, float* probs, int n,
                         void* stream);
int yk_net_destroy(yk_net_t* net);
/* Device-side check flags of this net's forwards since the last call (cleared by it; synchronises
 * the device): YK_NET_ERR_SYNC - a wave of the value head timed out waiting for v_head.2's columns
 * (its v row is then not trustworthy).  0 when every forward completed its hand-offs. */
#define YK_NET_ERR_SYNC 1u
int yk_net_errors(yk_net_t* net, uint32_t* flags);
/* Precision of every forward of this net (predict, leaf prior, the engine's expansions):
 * YK_PREDICT_F32 (default) - f32-equivalent products (fp16 hi/lo planes, three MFMAs each; within
 * 1e-5 of the reference's float32 CPU path); YK_PREDICT_F16 - fp16 weights and GEMM inputs with
 * f32 accumulation, one MFMA per product: the operand precision of the reference's own GPU
 * predict under autocast('cuda') (yacht/NNet.py:186-189), but with f32 outputs - the Linear
 * outputs and bias adds stay f32 where autocast rounds them to fp16, so it is closer to float32
 * than autocast is and not bit-equal to it.  LayerNorm, SiLU, softmax and tanh stay f32. */
#define YK_PREDICT_F32 0
#define YK_PREDICT_F16 1
int yk_net_set_precision(yk_net_t* net, int mode);

/* ---------------------------------------------------------------- held-out evaluation
 * A forward without dropout and, over its raw logits, YK_EVAL_COLS float64 numbers per example.  Not in the
 * reference; opt-in (Coach args.holdoutEps, python -m yacht_amd.evaluate).
 *
 * The raw pi_head output: DEVICE logits[n][3264] (columns >= 3226 unspecified) and v[n] = tanh(v_head), in
 * the net's current precision mode; exp(log_softmax(logits[i][:3226])) is yk_net_predict's pi.
 * Asynchronous on `stream`. */
int yk_net_logits(yk_net_t* net, const yk_state_t* states, float* logits, float* v, int n, void* stream);
/* The metrics over logits the caller supplies (DEVICE logits[n][ld], ld >= 3226, and v[n]).  Row i belongs to
 * example r = batch_idx[i] (i when batch_idx is NULL); DEVICE states (canonical boards), targets, values
 * and the policy CSR (pi_indptr[.. + 1], pi_cols, pi_vals float64; all three or all NULL) are indexed by r.
 * With x the row's 3226 logits, t = targets[r], z = values[r], (c_k, p_k) the CSR row, all arithmetic float64
 * (x, v, z widened from float32, every operation rounded on its own), rows[i][0..15] =
 *    0 lse = m + log(s), m = max x, e_a = exp(x_a - m), s = sum e_a
 *    1 lse - x_t, the hard cross-entropy (0 when t is outside 0..3225)
 *    2 the target's rank: #{a : x_a > x_t, or x_a == x_t and a < t} (3226 when t is outside)
 *    3 the policy's entropy lse - (sum e_a x_a) / s
 *    4 the policy's mass on getValidMoves(state r, 1): (sum over valid a of e_a) / s
 *    5 S = sum p_k          6 the soft cross-entropy sum p_k (lse - x[c_k]) over the entries with 0 <= c_k < 3226
 *    7 the target's entropy -sum over p_k > 0 of p_k log p_k               (5 - 7: 0 without a CSR)
 *    8 v    9 d = v - z    10 d * d    11 1.0 when v * z > 0    12 1.0 when col 2 == 0    13 1.0 when col 2 < 5
 *    14 1.0 when t is outside 0..3225    15 1.0
 * NaN or infinite logits propagate into the row.  HOST sums[16] = the column sums in an order fixed by n:
 * partial j (0..255) of a column is the sequential sum, from 0.0, of rows j, j + 256, j + 512, ... ascending, and
 * the sum is the sequential sum, from 0.0, of partials 0..255 ascending - so equal inputs give equal bits.
 * DEVICE rows[n][16] may be NULL (only the sums are wanted; a temporary is used).  Synchronises `stream`.
 * NULL required pointers, n < 0, ld < 3226, a half-given CSR: YK_ERR_ARG before any device work; n == 0: YK_OK
 * with sums all zero. */
#define YK_EVAL_COLS 16
int yk_examples_metrics(const float* logits, int64_t ld, const float* v, const yk_state_t* states,
                        const int32_t* targets, const float* values, const int64_t* pi_indptr,
                        const int32_t* pi_cols, const double* pi_vals, const int32_t* batch_idx, int64_t n,
                        double* rows, double* sums, void* stream);
/* yk_net_logits + yk_examples_metrics over examples batch_idx[0 .. n-1] (0 .. n-1 when NULL), `chunk` rows at
 * a time (<= 0: 16384, about 214 MB of logits scratch, allocated once per call on `stream`); one reduction
 * over all n rows at the end.  rows and sums do not depend on chunk.  Arguments, errors and synchronisation as
 * yk_examples_metrics. */
int yk_net_evaluate(yk_net_t* net, const yk_state_t* states, const int32_t* targets, const float* values,
                    const int64_t* pi_indptr, const int32_t* pi_cols, const double* pi_vals,
                    const int32_t* batch_idx, int64_t n, int chunk, double* rows, double* sums, void* stream);
/* The two functions above over x' instead of x (the legal-move mask): x'_a = x_a where
 * action_valid(state r, 1, a), -inf elsewhere.  Arguments, the 16 columns, the reduction order, errors and
 * synchronisation are theirs; column 4 is then 1, the rank in column 2 counts valid actions only, the entropy
 * skips the terms with e_a = 0 (no 0 * -inf).  A target outside the valid set gives an infinite column 1, a
 * state without a valid action NaN. */
int yk_examples_metrics_legal(const float* logits, int64_t ld, const float* v, const yk_state_t* states,
                              const int32_t* targets, const float* values, const int64_t* pi_indptr,
                              const int32_t* pi_cols, const double* pi_vals, const int32_t* batch_idx, int64_t n,
                              double* rows, double* sums, void* stream);
int yk_net_evaluate_legal(yk_net_t* net, const yk_state_t* states, const int32_t* targets, const float* values,
                          const int64_t* pi_indptr, const int32_t* pi_cols, const double* pi_vals,
                          const int32_t* batch_idx, int64_t n, int chunk, double* rows, double* sums, void* stream);
/* The contract of masked training, checked on the device: row i (example r = batch_idx[i], or i) must have a
 * valid action, its hard target (targets, may be NULL: not checked) must be valid, and every CSR entry with
 * p > 0 (all three CSR pointers, or all NULL: not checked) must sit on a valid column.  One wavefront per row;
 * HOST *first_bad = the lowest offending i, or -1, and HOST *kind = why: 0 clean, 1 no valid action, 2 the hard
 * target invalid or outside 0..3225, 3 a CSR column with p > 0 invalid or outside (a row's first finding in
 * that order).  The result is a minimum over per-block findings: no atomics, no dependence on launch order.
 * Synchronises `stream`.  NULL states / first_bad / kind, n < 0 or > 2^31 - 1, a half-given CSR: YK_ERR_ARG before
 * anything touches the device; n == 0: clean. */
int yk_examples_check_legal(const yk_state_t* states, const int32_t* targets, const int64_t* pi_indptr,
                            const int32_t* pi_cols, const double* pi_vals, const int32_t* batch_idx, int64_t n,
                            int64_t* first_bad /* HOST */, int* kind /* HOST */, void* stream);

/* ---------------------------------------------------------------- weighted minibatch sampling
 * Which examples a train step sees, drawn with replacement from per-example weights: recency x policy
 * surprise.  Not in the reference; opt-in (NNetWrapper args.trainSteps / sampleRecency / sampleSurprise).
 * All arithmetic is float64, every operation rounded on its own in the order written here; no atomics; equal
 * inputs give equal bits.  n <= 2^31 - 1.
 *
 * The weights.  DEVICE rows[n][ld], ld >= 16, is yk_net_evaluate's per-row table (NULL allowed only when
 * surprise == 0); HOST seg_ptr[nseg + 1] (seg_ptr[0] = 0, seg_ptr[nseg] = n, nondecreasing: empty segments
 * allowed) and HOST seg_factor[nseg] (finite, >= 0) give every example its segment's factor; 1 <= nseg <= 64;
 * surprise = sigma in [0, 1].  Per example i, with S, c, h = rows[i][5], [6], [7]: k_i = max(0, (c - h) / S)
 * when S > 0 and the quotient is finite, else 0 (a negative KL from rounding, a NaN row and a row without a
 * policy are "no surprise", not errors).  K = the sum of the k_i in yk_examples_metrics' order (partial j of
 * 256 = the sequential sum from 0.0 of rows j, j + 256, ... ascending; K = the sequential sum from 0.0 of
 * partials 0..255), written to HOST *ksum (0 when rows is NULL).  s_i = 1.0 when surprise == 0 or K == 0,
 * else a = (double)n * k_i; b = a / K; c2 = surprise * b; s_i = (1.0 - surprise) + c2.  DEVICE
 * w[i] = seg_factor[segment of i] * s_i.  Synchronises `stream`. */
int yk_sample_weights(const double* rows, int64_t ld, const int64_t* seg_ptr, const double* seg_factor, int nseg,
                      double surprise, int64_t n, double* w, double* ksum, void* stream);
/* The cumulative distribution of DEVICE w[n] into DEVICE cdf[n] (not aliasing w), in an order fixed by n alone:
 * chunk c is elements 256 c .. min(256 c + 255, n - 1); L[i] = the sequential inclusive sum of i's chunk from
 * 0.0, ascending; O[0] = 0.0, O[c + 1] = O[c] + L[last element of c], sequentially; cdf[i] = O[c] + L[i];
 * HOST *total = cdf[n - 1].  cdf[last of c] is O[c + 1] exactly, so cdf is nondecreasing.  YK_ERR_RANGE when a
 * weight is negative or NaN, or the total is not finite and > 0 (cdf is then unspecified).  Synchronises. */
int yk_sample_cdf(const double* w, int64_t n, double* cdf, double* total, void* stream);
/* m draws located in DEVICE cdf[n] (nondecreasing, as yk_sample_cdf leaves it) into DEVICE idx[m]: draw
 * j = first + r, r = 0 .. m-1, is Philox4x32-10 with counter (j lo, j hi, key, 0x20000000) - counter word 3 is 0
 * for the game streams, 0x10000000 for the reanalysis, 0x30000000 for the playout schedule, 0x40000000 for the
 * symmetries and 0x80000000 | move for the root noise - under key
 * (seed lo, seed hi); x = x0 | x1 << 32, u = (x >> 11) * 2^-53 (the game streams' uniform); t = u * cdf[n - 1];
 * idx[r] = #{i : cdf[i] <= t} (numpy's searchsorted(cdf, t, 'right')), and where that is n (u * total can round
 * up to the total) the first i with cdf[i] >= cdf[n - 1].  An element whose weight is zero, or absorbed by
 * the running sum, is never drawn.  m == 0: YK_OK, nothing launched.  Asynchronous on `stream`.
 * All three: NULL pointers, n <= 0 or > 2^31 - 1, m < 0, ld < 16, seg_ptr not as above, a factor negative or
 * not finite, nseg outside 1..64, surprise outside [0, 1] or NaN: YK_ERR_ARG before anything touches the
 * device. */
int yk_sample_draw(const double* cdf, int64_t n, uint64_t seed, uint32_t key, uint64_t first, int64_t m, int32_t* idx,
                   void* stream);

/* ---------------------------------------------------------------- reanalysis
 * Examples of the replay window searched again with the current net (yk_mcts_search on their boards), their
 * policy rows replaced by the new search's visit distribution.  Not in the reference; opt-in (Coach
 * args.reanalyseFraction / reanalyseSims, replay.reanalyse).  The only float64 operation is one division per
 * entry, rounded on its own; everything else is integer.  No atomics on data; row offsets come from a
 * three-pass scan (per-block sums, a scan of the sums, the add) in which no workgroup waits for another; equal
 * inputs give equal bits.  All three synchronise `stream`.
 *
 * Which rows.  Row i of the call is example k = index_base + i (a global index into the window's examples,
 * mod 2^64).  Its draw is Philox4x32-10 with counter (k lo, k hi, key, 0x10000000) - counter word 3 is 0 for the
 * game streams, 0x20000000 for the sampling, 0x30000000 for the playout schedule, 0x40000000 for the symmetries
 * and 0x80000000 | move for the root noise - under key (seed lo, seed hi); x = x0 | x1 << 32, u = (x >> 11) * 2^-53 (the game streams' uniform).
 * Row i is chosen iff u < fraction: 0 chooses none, 1 all.  DEVICE idx[0 .. m-1] = the chosen i ascending
 * (at most `capacity` are written; idx == NULL: count only), HOST *m = their number.  YK_ERR_CAPACITY when idx is
 * given and m > capacity.  NULL m, n < 0 or > 2^31 - 1, a fraction outside [0, 1] or NaN, capacity < 0 with
 * idx: YK_ERR_ARG before anything touches the device.  n == 0: YK_OK, *m = 0, nothing launched. */
int yk_reanalyse_select(int64_t n, uint64_t index_base, uint64_t seed, uint32_t key, double fraction, int32_t* idx,
                        int64_t capacity, int64_t* m, void* stream);
/* Visit counts as policy rows.  DEVICE counts[n][3226] (what yk_mcts_search writes).  Row r's entries are the
 * actions a with counts[r][a] > 0, ascending (a negative count is not an entry); sum = the sequential float64
 * sum of those counts in ascending action order (below 2^43: exact, so any order gives the same bits);
 * pi_vals = (double)N / sum - yk_examples_policies' arithmetic for a temp-1 move; targets[r] (DEVICE, may be
 * NULL) = the lowest action among those with the largest count (yk_examples_from_records' rule), -1 for a row
 * without entries.  Such rows are counted in HOST *n_empty (may be NULL) and are not an error.  Two phases as
 * yk_examples_policies: DEVICE pi_indptr[n + 1] and HOST *nnz are always written (and targets, when given);
 * pi_cols == NULL stops there; else pi_cols[nnz], pi_vals[nnz] (YK_ERR_CAPACITY if nnz > nnz_capacity).
 * NULL pi_indptr / nnz, NULL counts with n > 0, n < 0 or > 2^31 - 1, pi_cols without pi_vals: YK_ERR_ARG before
 * anything touches the device. */
int yk_policies_from_counts(const int32_t* counts, int64_t n, int64_t* pi_indptr, int32_t* pi_cols, double* pi_vals,
                            int64_t nnz_capacity, int32_t* targets, int64_t* nnz, int64_t* n_empty, void* stream);
/* Rows of a CSR replaced.  The old CSR (indptr[n + 1], cols, vals), DEVICE idx[m] strictly ascending within
 * [0, n), and a new CSR of m rows (new_indptr[m + 1], new_cols, new_vals) -> the CSR (out_indptr[n + 1], out_cols,
 * out_vals; out_indptr[0] = 0) and HOST *nnz: row idx[j] is new row j, unless that row is empty - then the old
 * row is kept, so a failed search never deletes a target; every other row is the old row, bit for bit.
 * out_cols == NULL: out_indptr and *nnz only; else YK_ERR_CAPACITY if nnz > nnz_capacity.  m == 0 copies the old
 * CSR.  idx not strictly ascending or out of range is detected on the device: YK_ERR_RANGE, the outputs
 * unspecified (nothing is written outside them).  An output that is one of the inputs, NULL indptr /
 * out_indptr / nnz, NULL idx / new_indptr with m > 0, out_cols without out_vals or without the cols / vals it
 * copies from, n or m < 0 or > 2^31 - 1: YK_ERR_ARG before anything touches the device. */
int yk_policies_splice(const int64_t* indptr, const int32_t* cols, const double* vals, int64_t n, const int32_t* idx,
                       int64_t m, const int64_t* new_indptr, const int32_t* new_cols, const double* new_vals,
                       int64_t* out_indptr, int32_t* out_cols, double* out_vals, int64_t nnz_capacity, int64_t* nnz,
                       void* stream);

/* ---------------------------------------------------------------- self-play engine
 * Batched Coach.executeEpisode (Coach.py:34-72) over n_envs games in lock-step; every game
 * runs MCTS.getActionProb (MCTS.py:28-54) / MCTS.search (MCTS.py:56-164) with its own
 * tree (reset per episode, Coach.py:93). */
typedef struct {
    int n_envs;             /* games per batch (per GPU) */
    int sims;               /* numMCTSSims */
    double cpuct;           /* cpuct */
    int temp_threshold;     /* tempThreshold */
    int max_moves;          /* record capacity per game (every real game has 48 moves) */
    int prior;              /* 0 = yk_net (MLP), 1 = hash prior (test) */
    int record_predictions; /* test: keep every expansion's (Ps * valids, v, leaf) of sampled games */
    int max_expansions;     /* capacity of that record per game (record_predictions only) */
    int64_t arena_entries;  /* per game per generation P/edge-slot entries; 0 = default */
    int record_stride;      /* record_predictions samples games e with e % record_stride == 0 (0 = 1:
                               every game); recording never changes the search path */
    int groups;             /* game groups, each on its own stream so that one group's forward runs
                               beside another's expand (results do not depend on it); 0 = auto
                               (2 with the net prior at >= 8192 games, else 1), at most 8 */
    int dual_trees;         /* arena: two trees per game, so MCTS vs MCTS plays two MCTS objects with
                               their own trees and nets (Coach.py:117-125's pmcts / nmcts) */
    double dirichlet_alpha; /* AlphaZero's root exploration noise, a departure from the reference, opt-in: on */
    double dirichlet_eps;   /* when alpha > 0 and eps > 0 (default 0, 0: off).  yk_selfplay then replaces each
                               real move's root prior once, before any UCB scan of that root in the move, by
                               P'[j] = float32((1 - eps) * (double)P[j] + eps * eta[j]) over the root's valid
                               actions j (ascending), eta ~ Dir(alpha) = yk_dirichlet_noise(seed, env id, move, V,
                               alpha).  yk_arena and yk_mcts_search never add noise.  The game's draw stream is
                               not consumed.  alpha NaN or < 0, eps outside [0, 1]: YK_ERR_ARG */
    int record_root_values; /* the search's own value of every real move, a departure from the reference, opt-in
                               (0 = off: no extra launch, info[..][7] stays 0).  On, yk_selfplay (never yk_arena or
                               yk_mcts_search) evaluates, after the last simulation of move m of game e, over the
                               edges (s, a) of the move's root with N > 0 in ascending action order (the
                               reference's Nsa / Qsa of the root, visits kept from earlier moves included)
                                   num = 0.0; den = 0.0                                     (float64)
                                   num = num + (double)N * Q ;  den = den + (double)N       (each edge)
                                   q32 = (float)(num / den)                                 (nearest even)
                               every operation rounded on its own (no FMA), N the edge's full count, Q its stored
                               float64 whatever its Python kind.  info[e][m][7] = the bit pattern of q32, +0 and
                               -0 both as 0x80000000: a recorded value is never the zero word, and a zero word
                               means "no value recorded" (flag off, a root not in the tree, den == 0 - the last
                               two are existing error states - and every move past the game's end).  The search,
                               the game streams and every other record are unchanged.  DESIGN.md section 7b-val */
} yk_engine_config_t;

typedef struct yk_engine yk_engine_t;
int yk_engine_create(yk_engine_t** eng, const yk_engine_config_t* cfg, yk_net_t* net);
int yk_engine_destroy(yk_engine_t* eng);
/* Plays one complete episode for each of the n_envs games (game i uses stream env_base+i).
 * Synchronises `stream` once per real move to test termination.  Returns YK_OK, or
 * YK_ERR_CAPACITY / YK_ERR_STATE if a device-side check failed (see yk_engine_stats). */
int yk_selfplay(yk_engine_t* eng, uint64_t seed, uint32_t env_base, void* stream);
/* Playout cap randomization (KataGo), a departure from the reference, opt-in; DESIGN.md section 6e.  Off
 * (fast_sims = 0, the state of a new engine): every real move of yk_selfplay runs `sims` simulations.  On
 * (fast_sims > 0): move m (0-based) of a yk_selfplay batch started with (seed, env_base) is a FULL move iff
 * u < full_prob, u = ((x0 | x1 << 32) >> 11) * 2^-53 of Philox4x32-10 under key (seed lo, seed hi) with counter
 * (m, env_base, 0, 0x30000000) - one draw per (batch, move), made on the host: all games of a batch are at the
 * same move, so the lock-step loop itself runs fewer simulations; no game stream is consumed.  Every other
 * move is a FAST move: fast_sims simulations instead of `sims`, no Dirichlet noise (its rows of
 * yk_engine_root_priors stay zero), and info[e][m][6] = status | YK_REC_FAST.  Everything else is as before -
 * the persistent tree, the temperature rule, the draws of the real step, the root value of
 * record_root_values (a fast move's is recorded: TD(lambda) targets of earlier full moves read it).  A
 * simulation is yk_mcts_search's: a batch's moves are that entry point's searches with sims = the move's cap.
 * yk_arena and yk_mcts_search are never capped.  The cap lives in the engine, not in yk_engine_config_t, whose
 * layout stays as it is.  fast_sims < 0, or on and not 2 <= fast_sims <= sims (one simulation on a fresh root
 * leaves every visit count zero, and a temp-1 move cannot be sampled from that) or full_prob outside [0, 1] or
 * NaN: YK_ERR_ARG, the engine unchanged.  Touches no device memory. */
#define YK_REC_FAST 0x100 /* info[..][6] of a fast move: the step status (YK_ST_*, 0..5) | this bit */
int yk_engine_set_playout_cap(yk_engine_t* eng, int fast_sims, double full_prob);
/* The schedule itself, the bits yk_selfplay uses: HOST full[m] = 1 when move m of a batch started with (seed,
 * env_base) is a full move under full_prob, else 0, m = 0 .. n_moves-1.  NULL full, n_moves < 0, full_prob
 * outside [0, 1] or NaN: YK_ERR_ARG.  Host only. */
int yk_playout_schedule(uint64_t seed, uint32_t env_base, double full_prob, int n_moves, uint8_t* full /* HOST */);
/* Forced playouts and policy target pruning (KataGo, Wu 2019 section 3.2), a departure from the reference,
 * opt-in; DESIGN.md section 6f.  Off (k = 0, the state of a new engine): nothing changes.  On (k > 0), at the
 * root (depth 0) of every FULL move of yk_selfplay - a fast move of the playout cap is neither forced nor
 * pruned, the rule of the root noise; yk_arena, yk_mcts_search and interior nodes never are.  Doubles unless
 * it says float; Ns the root's visit count, P[a] the float prior the search uses (the noised one under root
 * noise), N[a] / Q[a] the edge's count and value, c = cpuct:
 *   Forcing, at every simulation's root pick: a visited edge (N > 0) with N * N < (k * P) * Ns has u = +inf;
 *     nothing else in the scan changes (the first maximum in ascending action order wins).
 *   Pruning (prune = 1), once after the move's last simulation: c* = the visited edge with the largest N (the
 *     lowest action among equals) keeps its count; PUCT* = Q[c*] + (c * P[c*]) * sqrt(Ns) / (1 + N[c*]).  Every
 *     other visited edge: f = the largest integer with f * f <= (k * P) * Ns; from n = N, n is decremented
 *     while n > 0, N - n < f and Q + (c * P) * sqrt(Ns) / (1 + (n - 1)) < PUCT*; an n brought to exactly 1 that
 *     way becomes 0.  The pruned counts are what the move's record holds (visits, info[5]; edges at 0 leave the
 *     list) and what the real move is drawn from under both temperature rules; info[4] stays the raw Ns, and
 *     the tree keeps its raw N and Q.  The record image and its size are unchanged.
 * prune = 0 forces without pruning (tests, ablation).  Lives in the engine, not in yk_engine_config_t.
 * k < 0, NaN or infinite, or prune outside {0, 1}: YK_ERR_ARG, the engine unchanged.  Touches no device memory. */
int yk_engine_set_forced_playouts(yk_engine_t* eng, double k, int prune);
/* The pruning alone, on n rows given as a CSR: DEVICE indptr[n + 1], and per entry cols (the action), counts
 * (N; an entry with N <= 0 is no visited edge and keeps its word), q (Q), p (P); per row ns[n] (Ns, negative
 * taken as 0) -> DEVICE out[nnz], the pruned counts (out is none of the inputs).  c* of a row: the largest count, the
 * lowest column among equals.  k = 0 copies.  One wavefront per row; no atomics on data; equal inputs give
 * equal bits.  A NULL pointer, n < 0, k negative, NaN or infinite: YK_ERR_ARG before anything touches the
 * device.  An indptr that starts below 0 or decreases (or a row of more than 2^31 - 1 entries), detected on the
 * device before any row is read: YK_ERR_RANGE, out untouched.  Synchronises `stream`. */
int yk_policy_prune(const int64_t* indptr, const int32_t* cols, const int32_t* counts, const double* q, const float* p,
                    const int32_t* ns, int64_t n, double k, double cpuct, int32_t* out, void* stream);
/* First-play urgency (FPU reduction: Leela, KataGo), a departure from the reference, opt-in; DESIGN.md section
 * 6g.  Off (on = 0, the state of a new engine): nothing changes.  On, in EVERY search of this engine - yk_selfplay
 * (full and fast moves), yk_arena (both trees of a dual-tree engine) and yk_mcts_search - at every node with
 * Ns > 0 that has a visited and an unvisited valid edge.  Doubles and integers unless it says float; c32 =
 * f32(cpuct), sq = f32(sqrt(Ns)), sqe = f32(sqrt(Ns + 1e-8)):
 *   visited candidate    the largest u = f32(Q) + ((c32 * P) * sq) / f32(1 + N), the lowest compact index among
 *                        equals (a forced edge's u is +inf, as without the rule)
 *   unvisited candidate  the largest x = (c32 * P) * sqe over the unvisited edges, the lowest index among equals
 *   parent estimate      over the visited edges: W = sum N * llrint(Q * 2^32) (int64, ties to even), Mi = sum
 *                        (uint64)((double)P * 2^40) (truncated); fq = (float)((W / Ns) / 2^32 - r * sqrt(Mi / 2^40)),
 *                        r = root_reduction at depth 0 of a search and `reduction` elsewhere
 *   winner               the larger of the visited u and fq + x (one f32 add), the lower index on equality
 * A node at Ns = 0 and a node whose valid edges are all visited are scanned as without the rule.  The parent
 * estimate is the children's visit-weighted mean, not the node's own net value (the node record has no room
 * for one).  reduction = 0 is legal and is not off.  Lives in the engine, not in yk_engine_config_t.
 * NULL engine, or a reduction that is negative, NaN or infinite: YK_ERR_ARG, the engine unchanged.  Touches no
 * device memory. */
int yk_engine_set_fpu(yk_engine_t* eng, int on, double reduction, double root_reduction);
/* The rule's pick alone, on n nodes given as a CSR: DEVICE indptr[n + 1], and per entry p (P, float), counts
 * (N; an entry with N <= 0 is an unvisited edge), q (Q, read where N > 0); per row ns[n] (Ns, negative taken as
 * 0) -> DEVICE pick[n], the picked entry's index within its row (-1: an empty row), and unvisited[n], 1 when
 * that entry is an unvisited edge.  A row at Ns = 0, or with one kind of edge only, takes the plain argmax
 * over u and x (the lowest index among equals).  The same device functions as the search kernels; one
 * wavefront per row; no atomics on data; equal inputs give equal bits.  A NULL pointer, n < 0, a reduction
 * negative, NaN or infinite, a cpuct that is not finite, or outputs that alias counts, ns or each other:
 * YK_ERR_ARG before anything touches the device.  An indptr that starts below 0 or decreases (or a row of more
 * than 2^31 - 1 entries), detected on the device before any row is read: YK_ERR_RANGE, the outputs untouched.
 * Synchronises `stream`. */
int yk_fpu_pick(const int64_t* indptr, const float* p, const int32_t* counts, const double* q, const int32_t* ns,
                int64_t n, double cpuct, double reduction, int32_t* pick, int32_t* unvisited, void* stream);
/* The score-margin utility (KataGo's score utility), a departure from the reference, opt-in; DESIGN.md section
 * 6i.  Off (on = 0, the state of a new engine): nothing changes.  On, in EVERY search of this engine - yk_selfplay
 * (full and fast moves), yk_arena (both trees of a dual-tree engine) and yk_mcts_search - at the one place a
 * terminal value enters the search.  For a terminal state s, that is game_ended(s, 1) != 0, seen from `player`
 * (+1 / -1), with w = weight in [0, 1] and c = scale, finite and > 0, in game points (a pip is 1000 points):
 *   z = game_ended(s, player)                              (+-1; 1e-4 for a draw, for either player)
 *   m = total_with_bonus(s, 0) - total_with_bonus(s, 1)    (int)
 *   x = (double)(player * m) / c
 *   g = x / (1.0 + fabs(x))
 *   u = (1.0 - w) * z + w * g
 * Every operation is one IEEE double operation, rounded on its own (no FMA; 1.0 - w is computed once on the
 * host, the division is by c and not a multiplication by 1 / c), so numpy float64 gives the same bits; the squash
 * is rational because division and addition are correctly rounded, which a device tanh does not promise.
 * |u| <= 1.  A state is terminal when game_ended != 0, never when u != 0: at w = 1 a draw has u = 0 and is still
 * terminal.  A descent that reaches a terminal state returns -u(s, 1) on the canonical board, still typed as a
 * Python float; nothing else in the descent, the backup, the root scan, the node summaries, first-play urgency,
 * forced playouts or the root value changes.  The records (values, the final result and totals) and the arena
 * results stay the game's own.  weight = 0 is legal, is not off, and searches bit for bit as off does.  Lives in
 * the engine, not in yk_engine_config_t.  NULL engine, a weight outside [0, 1], a scale <= 0, NaN or infinite
 * values: YK_ERR_ARG, the engine unchanged.  Touches no device memory. */
int yk_engine_set_score_utility(yk_engine_t* eng, int on, double weight, double scale);
/* The rule alone, on n states given by the caller - the sibling of yk_ended: DEVICE states[n], players[n]
 * (+1 / -1) -> DEVICE u[n], the utility of state i seen from players[i] and 0.0 where the state is not terminal,
 * and margin[n] (may be NULL) = m, written for every state.  The same device function as the search kernels and
 * the value targets; one thread per state; no atomics; equal inputs give equal bits.  The setter's checks on
 * weight and scale, n < 0, or (n > 0) a NULL states, players or u: YK_ERR_ARG before anything touches the
 * device.  Asynchronous on `stream`. */
int yk_score_utility(const yk_state_t* states, const int32_t* players, int n, double weight, double scale, double* u,
                     int32_t* margin, void* stream);
/* The two self-play temperatures (AlphaZero / KataGo), a departure from the reference, opt-in; DESIGN.md
 * section 6h.  Off (the state of a new engine): nothing changes.  Both follow one schedule shape over the
 * 0-based index m of the real move, in host float64:
 *   T(m) = final + (early - final) * 2^(-m / halflife)          (early == final: T(m) = final, no halflife needed)
 * The host builds each table (max_moves doubles, yk_temperature_schedule) and uploads it; the kernels read
 * T and never evaluate the schedule.
 * Move-selection temperature (move_early, move_final), on the moves yk_selfplay draws at temp 1 today - real
 * move m with m + 1 < temp_threshold; the moves from there on stay the argmax path: with T = T(m) and the
 * recorded visit list n_0 .. n_(k-1) in ascending action order (the pruned list with forced playouts),
 *   w_i = pow((double)n_i, 1.0 / T), total = the left-to-right sum of w_i, c_i = c_(i-1) + w_i / total,
 *   last = c_(k-1), u = the game stream's next uniform53, the move = the first i with c_i / last > u
 * - today's draw with w in place of the counts: one uniform is consumed, so the stream position after the move
 * does not depend on T.  T == 1.0 exactly runs today's kernel.  info[0] stays 1; T is not recorded.
 * Root policy temperature (root_early, root_final), where the root noise is or would be applied - every move of
 * yk_selfplay, with the playout cap its full moves: the root's stored prior over its compact valid set
 * becomes, in place and once per move, with T = T(m),
 *   w_j = pow((double)P_j, 1.0 / T), S = sum w_j (float64), P'_j = (float)(w_j / S)
 * before any UCB scan of that root in the move (the noise's two phases).  With the noise also on, the same
 * launch then mixes from the rounded P': P''_j = (float)((1 - eps) * (double)P'_j + eps * eta_j), eta
 * unchanged.  T == 1.0 exactly, or weights that do not sum to > 0, leave P untouched.
 * Neither is applied by yk_arena, yk_mcts_search or the reanalysis, and neither changes the recorded visit
 * counts (the policy targets).  The schedules live in the engine, not in yk_engine_config_t.
 * A pair (early, final) of zeros: that schedule is off.  Otherwise move temperatures outside [0.05, 100] (visit
 * counts are 16-bit: 65535^20 is finite in float64), root temperatures outside [0.25, 10], a halflife that is
 * negative, NaN or infinite, or a halflife of 0 while a schedule that is on has early != final: YK_ERR_ARG, the
 * engine unchanged.  Waits for the device; keeps both tables on the host and on the device. */
int yk_engine_set_temperatures(yk_engine_t* eng, double move_early, double move_final, double root_early,
                               double root_final, double halflife);
/* HOST move_t[max_moves], root_t[max_moves] (either may be NULL): the tables the engine holds; zeros for a
 * schedule that is off. */
int yk_engine_temperatures(yk_engine_t* eng, double* move_t, double* root_t);
/* The schedule itself, the doubles the engine uploads: HOST out[m] = T(m), m = 0 .. n_moves-1, with the host
 * libm's pow.  NULL out, n_moves < 0, early or final not finite and > 0, halflife negative, NaN or infinite,
 * or 0 with early != final: YK_ERR_ARG.  Host only. */
int yk_temperature_schedule(double early, double final_t, double halflife, int n_moves, double* out /* HOST */);
/* The move draw alone, on n rows given as a CSR: DEVICE indptr[n + 1], counts per entry (a count below 0 is taken
 * as 0), and per row temps[n] (T) and u[n] (the uniform) -> DEVICE pick[n], the drawn entry's index within its
 * row (-1: an empty row or counts that are all 0), and total[n], the sum of w.  The same device function as
 * k_move_end's; one wavefront per row, 64 entries' pow at a time, the sums sequential; no atomics; equal inputs
 * give equal bits.  A NULL pointer, n < 0, or outputs that alias inputs: YK_ERR_ARG before anything touches the
 * device.  An indptr that starts below 0 or decreases (or a row of more than 2^31 - 1 entries), or a T that is
 * not finite and > 0, detected on the device before any row is read: YK_ERR_RANGE, the outputs untouched.
 * Synchronises `stream`. */
int yk_temperature_pick(const int64_t* indptr, const int32_t* counts, const double* temps, const double* u, int64_t n,
                        int32_t* pick, double* total, void* stream);
/* The root prior transform alone, on n rows: DEVICE p[n][3226], row i compact over its first nvalid[i] entries
 * (clamped to 0 .. 3226), temps[n] -> DEVICE out[n][3226], P' over those entries and 0 past them.  The same
 * device function as the engine's, so the same bits.  A NULL pointer, n < 0 or out == p: YK_ERR_ARG; a T that
 * is not finite and > 0: YK_ERR_RANGE, out untouched.  Synchronises `stream`. */
int yk_root_temper(const float* p, const int32_t* nvalid, const double* temps, int n, float* out, void* stream);
/* Per-kernel timing with HIP events on the engine's stream; resets the accumulators.
 * enable = 0 off, k > 0 on: the per-move launches are timed every time, the per-simulation
 * forward / expand pair in every k-th simulation of a move (1 = all; an event record between
 * dependent launches costs GPU time, so a stride keeps the timed batch's rate).
 * yk_engine_kernel_times (launches counts the timed ones): HOST ms[8],
 * launches[8] for classes 0 first descent of a move, 1 forward (the whole predict), 2 unused,
 * 3 expand + backup + the next descent, 4 move begin (root / tree compaction), 5 move end
 * (policy, sampling, real step), 6 the root noise and the root policy temperature, which share their launches
 * (both launches of a move; 0 launches when both are off - with one on and full root scans, simulation 1's descent is its own launch, timed as class 2),
 * 7 the root value (one launch per move after the move end; 0 launches without record_root_values). */
int yk_engine_profile(yk_engine_t* eng, int enable);
int yk_engine_kernel_times(yk_engine_t* eng, double* ms, int64_t* launches);
/* HOST out[16]: 0 expansions, 1 valid entries scanned by UCB, 2 real moves (max over games),
 * 3 device error flags, 4 max live nodes, 5 max live edges, 6 max arena entries used (per shard),
 * 7 new-node valid entries written, 8 search path edges backed up, 9 lock-step sims run,
 * 10-13 node / edge / arena / visit capacities, 14 game groups, 15 forward head parts (workgroups per 16-row tile) */
int yk_engine_stats(yk_engine_t* eng, int64_t* out);
/* Further counters of the last batch, summed over games; writes out[0 .. n-1] of:
 * 0 edges gathered by the UCB scans (one 16-B edge per visited entry scanned, MCTS.py:122-133; with
 *   stats 1 and 7-8 the expand's algorithmic bytes, bench.py roofline_env)
 * 1-3 expansions whose prior took the window, the sparse and the general path (their sum: stats 0;
 *   YK_PRIOR_FAST=0 sends every one through the general path with the gather P write, =1 keeps the window
 *   and sparse paths and leaves the general path's P write unstaged, =2 stages it after the dense pass; unset
 *   or anything else, a general leaf at 10 dice also computes its priors compact-first through the window -
 *   still counted as general)
 * 4 lock-step moves of the last batch that ran with the fast playout cap (0 with the cap off, and after yk_arena)
 * 5 root picks of the last batch that took a forced edge, 6 visits its pruning took off the recorded counts
 *   (yk_engine_set_forced_playouts; both 0 with it off, and after yk_arena)
 * 7 descent picks of the last batch (every depth) that first-play urgency gave to the unvisited candidate,
 *   8 picks its rule decided: nodes with both kinds of edge (yk_engine_set_fpu; both 0 with it off)
 * 9 descents of the last batch that ended at a terminal state and returned a score-margin utility
 *   (yk_engine_set_score_utility; 0 with it off - the default instantiations do not count) */
int yk_engine_counters(yk_engine_t* eng, int64_t* out, int n);
/* Copies the last episode batch to HOST arrays (any may be NULL):
 *   states[n][max_moves][8]  canonical board of each example (Coach.py:57,61)
 *   info[n][max_moves][8]    temp, player, action, expansions-so-far, root Ns, n visited, status (| YK_REC_FAST
 *                            for a fast move of the playout cap), 0 (the move's root value word with
 *                            record_root_values, see yk_engine_config_t)
 *   ctr[n][max_moves][2]     stream counter before the search / before the real step
 *   values[n][max_moves]     example value r*(-1)**(player != curPlayer) (Coach.py:72)
 *   final_states[n][8], n_moves[n]
 *   visits_off[n*max_moves+1], visits[...][2] (action, N): root visit counts, ascending
 *   action (size: yk_engine_records(...) with visits=NULL returns the total in *n_visits). */
int yk_engine_records(yk_engine_t* eng, uint64_t* states, int32_t* info, uint64_t* ctr, double* values,
                      uint64_t* final_states, int32_t* n_moves, int64_t* visits_off, int32_t* visits,
                      int64_t* n_visits);
/* record_predictions, for the R = ceil(n_envs / record_stride) sampled games (game r * record_stride):
 * HOST pi[R][max_expansions][3226] = the prior each expansion was made with, masked (MCTS.py:86-88:
 * Ps * valids, before the renormalisation, the production valid-only softmax of yk_net_leaf_prior),
 * v[R][max_expansions], leaves[R][max_expansions] the expanded canonical states, count[R] the
 * expansions of each game (> max_expansions: the record was truncated).  Any may be NULL. */
int yk_engine_predictions(yk_engine_t* eng, float* pi, float* v, yk_state_t* leaves, int32_t* count);
/* Root noise of the last yk_selfplay, for the R record_predictions games: HOST before[R][max_moves][3226],
 * after[R][max_moves][3226] (either may be NULL), dense by action - the prior P of move m's root as the
 * noise found it and P' as it left it, 0 at invalid actions and for moves >= the game's n_moves.
 * With the root policy temperature on (yk_engine_set_temperatures) `before` is the prior before the tempering
 * and `after` what the search scans: the tempered prior, or with the noise also on its mix.
 * YK_ERR_STATE unless the engine has record_predictions and the noise or the root policy temperature on and has
 * played a batch. */
int yk_engine_root_priors(yk_engine_t* eng, float* before, float* after);
/* test: HOST p[3226] = the prior P stored in the tree for the root of game `game`'s current move (tree
 * `game`), dense by action, 0 at invalid actions: what the expansion wrote (MCTS.py:90-107) and the UCB scans
 * read.  YK_ERR_STATE while no descent of the move has found the root in the tree (before the move's second
 * simulation on a fresh tree). */
int yk_engine_root_prior(yk_engine_t* eng, int game, float* p);
/* The noise itself: eta[i*3226 + j], j < nvalid[i], is the Dirichlet(alpha) sample over nvalid[i] valid
 * actions that game env_ids[i] gets at move moves[i] under `seed` (0 for j >= nvalid[i]; nvalid is clamped
 * to 0..3226) - the same device function as the engine's, so the same bits.  Defined by Philox4x32-10 with
 * counter (draw i, action j, env, 0x80000000 | move) - the game streams use counter word 3 = 0 - and, in
 * float64, u = ((x >> 11) + 0.5) 2^-53, a Marsaglia-Tsang gamma per action (alpha < 1: boosted by
 * u^(1/alpha)) and eta = g / sum g (1 / nvalid when the sum is 0); DESIGN.md section 6d.  DEVICE arrays
 * env_ids[n], moves[n], nvalid[n], eta[n][3226]; alpha > 0. */
int yk_dirichlet_noise(uint64_t seed, const uint32_t* env_ids, const int32_t* moves, const int32_t* nvalid,
                       double alpha, double* eta, int n, void* stream);
/* Fixed-size trajectory records of the last batch for the multi-GPU all-gather:
 * yk_engine_record_bytes = size of the packed image; yk_engine_pack_records copies it
 * (device to device, async on `stream`) into dst (device, >= that many bytes).  Image:
 * states[n][M][8] u64 | info[n][M][8] i32 | ctr[n][M][2] u64 | values[n][M] f64 |
 * visits[n][VCAP] u32 (action << 16 | N) | visits_off[n][M+1] i32 | n_moves[n] i32 |
 * final_states[n][8] u64 (M = max_moves, VCAP = 2 * M * max(sims, 32)). */
int64_t yk_engine_record_bytes(yk_engine_t* eng);
int yk_engine_pack_records(yk_engine_t* eng, void* dst, int64_t capacity, void* stream);

/* The replay buffer's examples: n_images packed record images back to back (each
 * yk_engine_record_bytes of an engine with n_envs games, max_moves, sims - e.g. every rank's image
 * after the all-gather) -> one example per move of the first n_games games (image-major; < 0 = all),
 * in (image, game, move) order: Coach.executeEpisode's (canonicalBoard, pi, v) (Coach.py:57-72)
 * as NNetWrapper.train consumes it - states[k] the board, targets[k] = argmax(pi) (NNet.py:145-146:
 * the played action at temp 0, the most visited action at temp 1, lowest on ties), values[k] = v
 * (float32).  The first `skip` examples are dropped (the maxlenOfQueue deque keeps the last ones,
 * Coach.py:86-90); at most `capacity` are written.  states = NULL: count only.  HOST *n_examples =
 * examples written (or countable).  Synchronises `stream`. */
int yk_examples_from_records(const void* images, int n_images, int n_envs, int max_moves, int sims,
                             int64_t n_games, int64_t skip, int64_t capacity, yk_state_t* states, int32_t* targets,
                             float* values, int64_t* n_examples, void* stream);
/* The full policies of the same examples (Coach.py:57-61: MCTS.getActionProb's pi, MCTS.py:44-54 -
 * one-hot at the played action at temp 0, N / sum N at temp 1) as a sparse CSR of their nonzero
 * entries, for the examples file (Coach.py:144-151) and code that iterates the reference's tuples.
 * Examples skip .. skip + n_examples - 1 (as yk_examples_from_records numbers them; n_examples <=
 * the examples after skip).  DEVICE pi_indptr[n_examples + 1] (always written: example k's entries
 * are pi_indptr[k] .. pi_indptr[k+1]-1), pi_cols[nnz] (actions, ascending), pi_vals[nnz] (float64),
 * values[n_examples] (float64 v, may be NULL).  pi_cols = NULL: count only.  HOST *nnz = the
 * entries (YK_ERR_CAPACITY if more than nnz_capacity).  Synchronises `stream`. */
int yk_examples_policies(const void* images, int n_images, int n_envs, int max_moves, int sims, int64_t n_games,
                         int64_t skip, int64_t n_examples, int64_t* pi_indptr, int32_t* pi_cols, double* pi_vals,
                         int64_t nnz_capacity, double* values, int64_t* nnz, void* stream);
/* Value targets from the search, a departure from the reference (whose example value is the outcome z,
 * Coach.py:71-72), opt-in: mixes each move's recorded root value into the target (beta) and / or bootstraps
 * from the later moves' root values, TD(lambda); DESIGN.md section 7b-val.  Images, n_games, skip and the
 * example numbering are yk_examples_from_records'; examples skip .. skip + n_examples - 1 are written
 * (n_examples > the examples after skip: YK_ERR_ARG).  The images must come from an engine with
 * record_root_values unless (beta, lambda) = (0, 1).  Per game with T recorded moves, t = 0 .. T-1:
 *   p_t = info[t][1] (+1 / -1), z_t = the recorded float64 value, q_t = (double) of the float32 whose bit
 *   pattern is info[t][7].  All arithmetic float64, every operation rounded on its own (no FMA):
 *     W_t = p_t * q_t ;  Z_t = p_t * z_t
 *     G_{T-1} = Z_{T-1} ;  G_t = (1.0 - lambda) * W_{t+1} + lambda * G_{t+1}      t = T-2 .. 0
 *     target_t = p_t * G_t
 *     v_t = (1.0 - beta) * target_t + beta * q_t ;  values[k] = (float)v_t       (nearest even, once)
 *   lambda == 1 skips the recursion: G_t = Z_t for every t, and no later root value is read.  beta == 0 skips
 *   the q_t term: v_t = target_t.  So (0, 1) is yk_examples_from_records' values bit for bit and needs no
 *   recorded root value.
 * DEVICE values[n_examples]; root_values[n_examples] (may be NULL) = q_t as float32, NaN (0x7FC00000) where the
 * word is 0.  The whole game is read even where skip or n_examples cut it.  A kept example whose formula
 * needs a root value that is absent (word 0) - its own when beta != 0, any later move's of its game when
 * lambda != 1 - is counted in HOST *n_missing (may be NULL); when the count is > 0 the call returns
 * YK_ERR_STATE and the outputs are unspecified.  beta or lambda outside [0, 1] or NaN, n_examples < 0, NULL
 * values with n_examples > 0, NULL images or a non-positive dimension: YK_ERR_ARG before anything touches the
 * device.  Synchronises `stream`. */
int yk_examples_value_targets(const void* images, int n_images, int n_envs, int max_moves, int sims,
                              int64_t n_games, int64_t skip, int64_t n_examples, double beta, double lambda,
                              float* values, float* root_values, int64_t* n_missing, void* stream);
/* yk_examples_value_targets under the score-margin utility (the rule at
 * yk_engine_set_score_utility): the same kernel, reading U_t wherever the formulas above read Z_t = p_t * z_t,
 *     g1  = the rule's g for player 1 from the game's final board in the images (one value per game)
 *     U_t = (1.0 - weight) * Z_t + weight * g1
 * so at (beta, lambda) = (0, 1) values[k] = (float)(p_t * U_t), no root value is read and none can be missing; at
 * other (beta, lambda) the recursion and the mix run on U.  The recorded root values are already in utility units
 * when the engine that played searched under the same knobs.  root_values and n_missing behave as above.  The
 * setter's checks on weight and scale, and every check of yk_examples_value_targets: YK_ERR_ARG before anything
 * touches the device.  weight = 0 gives yk_examples_value_targets' bits.  Synchronises `stream`. */
int yk_examples_utility_targets(const void* images, int n_images, int n_envs, int max_moves, int sims,
                                int64_t n_games, int64_t skip, int64_t n_examples, double beta, double lambda,
                                double weight, double scale, float* values, float* root_values, int64_t* n_missing,
                                void* stream);
/* The examples of full moves (playout cap).  Images, n_games and the example numbering
 * are yk_examples_from_records' with skip = 0.  DEVICE idx[0 .. n_full-1] = the numbers, ascending, of the
 * examples whose info[..][6] lacks YK_REC_FAST (at most `capacity` are written; idx == NULL: count only), HOST
 * *n_full = their count.  Images of an engine without the cap give 0 .. total-1.  YK_ERR_CAPACITY when idx is
 * given and n_full > capacity.  No atomics on data; the offsets come from the three-pass scan of the
 * reanalysis, in which no workgroup waits for another; equal inputs give equal bits.  NULL images or n_full, a
 * non-positive dimension, sims < 0, capacity < 0 with idx, more than 2^31 - 1 examples: YK_ERR_ARG (all but the
 * last before anything touches the device).  Synchronises `stream`. */
int yk_examples_full_rows(const void* images, int n_images, int n_envs, int max_moves, int sims, int64_t n_games,
                          int32_t* idx, int64_t capacity, int64_t* n_full, void* stream);
/* Rows of a CSR gathered.  The CSR (indptr[n + 1], cols, vals) and DEVICE idx[m], each within [0, n), in any
 * order and with repeats -> the CSR (out_indptr[m + 1], out_cols, out_vals; out_indptr[0] = 0) and HOST *nnz:
 * out row j is row idx[j], bit for bit.  Two phases as yk_policies_splice: out_cols == NULL writes out_indptr
 * and *nnz only; else YK_ERR_CAPACITY if nnz > nnz_capacity.  An idx outside [0, n) is detected on the device:
 * YK_ERR_RANGE, the outputs unspecified (nothing is written outside them).  m == 0: YK_OK, out_indptr[0] = 0,
 * *nnz = 0.  No atomics on data, offsets from the same scan, equal inputs give equal bits.  An output that is
 * one of the inputs, NULL indptr / out_indptr / nnz, NULL idx with m > 0, out_cols without out_vals / cols /
 * vals or with nnz_capacity < 0, n or m < 0 or > 2^31 - 1: YK_ERR_ARG before anything touches the device.
 * Synchronises `stream`. */
int yk_policies_take(const int64_t* indptr, const int32_t* cols, const double* vals, int64_t n, const int32_t* idx,
                     int64_t m, int64_t* out_indptr, int32_t* out_cols, double* out_vals, int64_t nnz_capacity,
                     int64_t* nnz, void* stream);
/* Symmetry augmentation of examples, a departure from the reference (whose getSymmetries is the identity),
 * opt-in: the game depends only on the multisets of the dice and is symmetric in the two auction groups,
 * while the features and the score actions are positional.  Row i of the call is example k = index_base + i
 * (a global index into the pooled examples); `flags` is a bit-set of YK_SYM_*; DESIGN.md section 7b-sym.
 *   Draws: draw d is Philox4x32-10 with counter (d, k & 0xffffffff, epoch_key, 0x40000000) - counter word 3
 *     is 0 for the game streams, 0x10000000 / 0x20000000 / 0x30000000 for the reanalysis, the sampling and the
 *     playout schedule, and 0x80000000 | move for the root noise - under key (seed lo, seed hi);
 *     below_d(m) = (x1 * m) >> 32 with x1 the output's word 1 (the game streams' rule).
 *   A list of length L with first draw b is permuted by perm = [0 .. L-1]; for m = L-1 .. 1:
 *     j = below_{b + (L-1-m)}(m + 1), swap perm[m], perm[j]; new[i] = old[perm[i]] (an old position p moves
 *     to perm^-1(p)).  First draws, fixed whatever the flags: p1 carry 0, p2 carry 16, rollA 32, rollB 40;
 *     the groups are exchanged iff x1 >> 31 of draw 48.
 *   YK_SYM_CARRY permutes both carries over their own lengths; YK_SYM_ROLLS each roll whose hasA / hasB bit
 *     is set; YK_SYM_GROUPS, after the rolls, exchanges the rollA / rollB fields and the two has bits and
 *     XORs 0x80 into each bid byte that is not 0xFF.  Every other bit of the 64 bytes is copied; phase and
 *     round are not consulted.  A flag that is off leaves its part the identity and moves no draw index.
 *   Actions (examples are canonical: the mover is p1), a bijection A_k of 0 .. 3225: phase 0 and a < 202:
 *     (a + 101) mod 202 when the groups were exchanged; phase 1 and 202 <= a, combo positions c0 < .. < c4
 *     with c4 < len(p1 carry): 202 + cat * 252 + index of sorted(perm1^-1(c)) in COMB_5_OF_10; else a.
 *   out_states[i] = the board; out_targets[i] = A_k(targets[i]); CSR row i (entries pi_indptr[i] ..
 *     pi_indptr[i+1]-1 of pi_cols / pi_vals, written at the same positions of out_cols / out_vals): the
 *     same entries under A_k in ascending new column order, each value with its entry.  pi_indptr is not
 *     copied.  Columns must lie in 0 .. 3225: another is skipped and its row's output is unspecified.
 * targets / out_targets may both be NULL, and so may the three CSR inputs with the two CSR outputs; out must
 * not alias in.  n < 0, flags outside 0 .. 7, a half-given pair, NULL states / out_states with n > 0:
 * YK_ERR_ARG before anything touches the device.  flags = 0 copies.  Asynchronous on `stream`. */
#define YK_SYM_CARRY 1
#define YK_SYM_ROLLS 2
#define YK_SYM_GROUPS 4
int yk_examples_augment(const yk_state_t* states, const int32_t* targets, const int64_t* pi_indptr,
                        const int32_t* pi_cols, const double* pi_vals, int64_t n, int64_t index_base, uint64_t seed,
                        uint32_t epoch_key, int flags, yk_state_t* out_states, int32_t* out_targets,
                        int32_t* out_cols, double* out_vals, void* stream);

/* ---------------------------------------------------------------- Arena
 * Batched Arena.playGame (Arena.py:30-93), n_envs games in lock-step: `agent` in seat
 * agent_seat[i] (HOST, [n]; 1 = moves first, -1) against `opponent` in the other seat, each a
 * YK_PLAYER_*: MCTS = np.argmax(MCTS.getActionProb(board, temp=0)) (Coach.py:124-125) with the
 * engine's net / prior and sims, one tree per game for the whole game; RANDOM =
 * RandomYachtPlayer (YachtPlayers.py:174-183); GREEDY = GreedyYachtPlayer (:186-214).  Game i
 * uses stream env_base+i for every draw.  Returns like yk_selfplay. */
#define YK_PLAYER_MCTS 0
#define YK_PLAYER_RANDOM 1
#define YK_PLAYER_GREEDY 2
int yk_arena(yk_engine_t* eng, uint64_t seed, uint32_t env_base, const int32_t* agent_seat, int agent, int opponent,
             void* stream);
/* HOST outputs of the last yk_arena (any may be NULL): result[n] = curPlayer * getGameEnded
 * (Arena.py:93, from player 1's view: +1 / -1 / +-1e-4 draw), totals[n][2] (player 1, player 2,
 * with bonus), n_moves[n], actions[n][max_moves] (-1 past the end), final_states[n][8],
 * rng_ctr[n] (stream counter at the end).  yk_engine_records also works after yk_arena. */
/* The opponent seat's net for MCTS vs MCTS arenas of a dual_trees engine (default: the engine's
 * net).  The gating arena of Coach.learn: yk_arena(agent = previous net's MCTS, opponent = new). */
int yk_engine_set_opponent_net(yk_engine_t* eng, yk_net_t* net);
int yk_arena_results(yk_engine_t* eng, double* result, int32_t* totals, int32_t* n_moves, int32_t* actions,
                     uint64_t* final_states, uint64_t* rng_ctr);

/* ---------------------------------------------------------------- MCTS plugin
 * MCTS(game, nnet, args).getActionProb (MCTS.py:28-54) for n_envs independent searches
 * sharing nothing: runs `sims` searches from roots[i] (device, canonical boards) with
 * persistent trees, drawing from game i's stream (rng_ctr[i], advanced), and writes the
 * root visit counts counts[i*3226 + a] (device).  Roots must not go back in round
 * (trees keep only nodes of rounds >= the root's, which is parity-safe because a game's
 * round never decreases).  yk_mcts_reset clears all trees. */
int yk_mcts_search(yk_engine_t* eng, const yk_state_t* roots, uint64_t seed, const uint32_t* env_ids,
                   uint64_t* rng_ctr, int sims, int32_t* counts, void* stream);
int yk_mcts_reset(yk_engine_t* eng);

/* ---------------------------------------------------------------- training
 * NNetWrapper.train (yacht/NNet.py:118-174): one optimiser step per minibatch of YachtNNet -
 * loss = cross_entropy(logits, argmax(pi)) + vloss_weight * mse(v, z) (:143-148),
 * clip_grad_norm_(max_grad_norm) (:152-153), AdamW(lr, weight_decay) (:109-110).  Two modes:
 * amp = 0, float32 (the reference's CPU path, :157-165); amp = 1, the reference's GPU path
 * (:113-116, 141-155): autocast('cuda') arithmetic (fp16 Linear layers with f32 accumulation,
 * f32 LayerNorm and losses) on fp16 MFMA kernels, loss scaling with GradScaler('cuda')
 * semantics (init_scale, x2 after growth_interval finite steps, x0.5 and the step skipped on an
 * inf / nan gradient), unscale before the clip.  Dropout masks come from the Philox stream
 * (seed, layer, step, row, column), not torch's generator; rows are numbered from the offset set
 * by yk_trainer_set_row_offset (0 by default; it applies to the next backward only and resets to 0
 * after it), so ranks splitting one minibatch draw the masks of the whole minibatch.  Parameters, gradients and Adam moments are flat device buffers in
 * state_dict order. */
typedef struct {
    int max_batch;          /* batch_size (rows per step, upper bound) */
    float lr, weight_decay; /* AdamW */
    float beta1, beta2, eps;
    float max_grad_norm;    /* 5.0 in the reference */
    float vloss_weight;     /* 1.5 in main.py */
    float dropout;          /* 0.3 in main.py; 0 for deterministic parity tests */
    uint64_t seed;          /* dropout stream */
    int amp;                /* 0: float32 step; 1: mixed precision (autocast + GradScaler) */
    float init_scale;       /* GradScaler init_scale (0: 65536) */
    int growth_interval;    /* GradScaler growth_interval (0: 2000) */
} yk_train_config_t;
typedef struct yk_trainer yk_trainer_t;
/* params: HOST float32 arrays in YachtNNet.state_dict() order (as yk_net_create) */
int yk_trainer_create(yk_trainer_t** t, int hidden, int nblocks, const float* const* params, int nparams,
                      const yk_train_config_t* cfg);
int yk_trainer_destroy(yk_trainer_t* t);
/* device pointers of the flat parameter and gradient buffers (for a DDP all-reduce of grads) */
int yk_trainer_buffers(yk_trainer_t* t, float** params, float** grads, int64_t* nparams);
/* forward + backward of one minibatch into the gradient buffer (overwritten).  Example i of the
 * batch is replay entry batch_idx[i] (device, or NULL for 0..batch-1): states[] packed canonical
 * boards, targets[] = argmax(pi) (NNet.py:145-146), values[] = v.  Losses: yk_trainer_losses. */
int yk_trainer_backward(yk_trainer_t* t, const yk_state_t* states, const int32_t* targets, const float* values,
                        const int32_t* batch_idx, int batch, void* stream);
/* clip_grad_norm_ + AdamW on the (possibly all-reduced) gradient buffer; advances the step */
int yk_trainer_apply(yk_trainer_t* t, void* stream);
/* yk_trainer_backward + yk_trainer_apply; in amp mode the gradient launches also sum the unscaled
 * grad norm (nothing can change the buffer between the two), so apply does not re-read it */
int yk_trainer_step(yk_trainer_t* t, const yk_state_t* states, const int32_t* targets, const float* values,
                    const int32_t* batch_idx, int batch, void* stream);
/* The same two calls with soft policy targets: the loss's policy term is cross_entropy(logits, pi)
 * with probability targets (mean over the batch) - the full MCTS visit policy instead of its
 * argmax; a departure from the reference (NNet.py:145-146), opt-in.  pi is the DEVICE CSR
 * yk_examples_policies writes: batch row i uses CSR row batch_idx[i] (row i when batch_idx is
 * NULL), entries pi_indptr[r] .. pi_indptr[r+1]-1, pi_cols ascending, pi_vals float64 - each
 * rounded to float32 once (as torch.as_tensor(pi).float()).  Per row, with s = the float32 sum of
 * its entries in CSR order: CE = sum_k p_k (lse - z[a_k]), dlogit[a] = (s softmax[a] - p[a]) / batch.
 * s is not assumed to be 1; a row without entries has CE 0 and no policy gradient; an entry whose
 * column is outside 0..3225 is ignored; a one-hot row (p = 1.0) is yk_trainer_backward's
 * arithmetic bit for bit.  Value loss, clip, AdamW, GradScaler and dropout as above;
 * yk_trainer_losses out[0] = sum_i CE_i.  NULL states / pi_indptr / pi_cols / pi_vals / values or
 * a batch outside 1..max_batch: YK_ERR_ARG, before anything touches the device. */
int yk_trainer_backward_soft(yk_trainer_t* t, const yk_state_t* states, const int64_t* pi_indptr,
                             const int32_t* pi_cols, const double* pi_vals, const float* values,
                             const int32_t* batch_idx, int batch, void* stream);
int yk_trainer_step_soft(yk_trainer_t* t, const yk_state_t* states, const int64_t* pi_indptr, const int32_t* pi_cols,
                         const double* pi_vals, const float* values, const int32_t* batch_idx, int batch,
                         void* stream);
/* HOST out[3]: sum over the last batch of cross-entropy, of squared value error; grad sq-norm */
int yk_trainer_losses(yk_trainer_t* t, double* out);
/* a reporting epoch's "Avg Loss" (NNet.py:150-160) without a host round trip per minibatch:
 * begin zeroes a device accumulator; every later yk_trainer_backward adds its batch's
 * ce/b + vloss_weight*se/b to it (one 1-thread launch on that stream) until end, which
 * synchronises and writes HOST out[2] = (sum of those batch losses, batches) */
int yk_trainer_epoch_loss_begin(yk_trainer_t* t, double vloss_weight);
int yk_trainer_epoch_loss_end(yk_trainer_t* t, double* out);
/* copy parameters (which 0), gradients (1), exp_avg (2), exp_avg_sq (3) to / from HOST arrays in
 * state_dict order (NULL entries skipped); set: step >= 0 also sets the optimiser step count */
int yk_trainer_get(yk_trainer_t* t, int which, float* const* out);
int yk_trainer_set(yk_trainer_t* t, int which, const float* const* in, int64_t step);
int64_t yk_trainer_step_count(yk_trainer_t* t);
/* the global row number of the next backward's first example (dropout masks; DDP ranks pass
 * their offset into the minibatch) */
int yk_trainer_set_row_offset(yk_trainer_t* t, int64_t row0);
/* HOST out[4] (amp mode): loss scale, growth tracker, optimiser steps taken, last step skipped */
int yk_trainer_amp_state(yk_trainer_t* t, double* out);

/* ---------------------------------------------------------------- legal-move mask (opt-in)
 * on = 1: every later yk_trainer_backward / _step and both _soft forms take the policy softmax, its loss and
 * its gradient over each row's valid actions only: L_i = {a : action_valid(states[idx[i]], 1, a)}, the logits
 * x'_a = x_a on L_i and -inf elsewhere (float32 trainer: x_a = z[a] + bpi[a]; mixed precision: the fp16-rounded
 * r16(acc + bias), masked after that rounding), CE = lse' - x'_t (soft: sum p_k (lse' - x'_{c_k})),
 * dlogit_a = (s softmax(x')_a - p_a) / B - exactly 0 outside L_i.  One more launch per backward writes the
 * rows' bits into a trainer-owned buffer (allocated by the first call with on = 1).  The caller keeps the
 * contract yk_examples_check_legal checks; the trainer does not defend it (an empty L_i gives NaN, a target
 * outside L_i an infinite cross-entropy).  on = 0 (the default): the launches of a trainer that never had the
 * mask.  Trainer state, not a field of yk_train_config_t.  NULL, or on outside {0, 1}: YK_ERR_ARG, nothing on
 * the device touched. */
int yk_trainer_set_legal_mask(yk_trainer_t* t, int on);

/* ---------------------------------------------------------------- averaged (EMA) weights (opt-in)
 * A shadow e of the trainer's flat parameter buffer p that follows it, for play and gating; a departure from
 * the reference, which plays the last minibatch's iterate.  Per element, in float32, each operation rounded
 * once and never fused:  e <- e + w * (p - e).
 *
 * The weight of update t (t = updates made so far, 0-based), computed on the host in double:
 *     d_t = min(decay, (1 + t) / (10 + t)),  w_t = (float)(1.0 - d_t)
 * (the min is a warm-up: the first updates are not dominated by the initial shadow).  A pure host function,
 * no device is touched.  decay outside [0, 1) or NaN, t < 0 or a NULL w: YK_ERR_ARG. */
int yk_ema_weight(double decay, int64_t t, float* w /* HOST */);
/* The kernel alone on caller-owned DEVICE buffers of n floats: ema[i] <- ema[i] + w * (params[i] - ema[i]).
 * One grid-stride streaming pass on `stream` (no synchronisation); 16-byte accesses when both pointers are
 * 16-byte aligned, scalar ones otherwise and for the tail - the pointers need float alignment only, and the
 * bits do not depend on the path or the grid.  n == 0: YK_OK without a launch.  NULL pointers, n < 0, w outside
 * [0, 1] or NaN: YK_ERR_ARG before anything touches the device. */
int yk_ema_update(float* ema, const float* params, int64_t n, float w, void* stream);
/* decay in (0, 1) with every >= 1 turns the average on: after every `every`-th yk_trainer_apply since the last
 * update (yk_trainer_step* included), on that apply's stream and after its update launches, the shadow moves by
 * w_t and the update is counted.  The first call that turns it on allocates the shadow (freed by
 * yk_trainer_destroy); turning it on - the first time or after it was off - copies the current parameters into
 * the shadow on the device and sets both counts to 0.  A call while it is on changes only the two knobs.
 * decay == 0 (every >= 1) turns it off: the shadow is no longer used and yk_trainer_apply's launches are
 * those of a trainer that never had one.  Anything else (NULL, decay < 0, >= 1 or NaN, every < 1): YK_ERR_ARG,
 * the trainer as it was.  Synchronises the device when it copies.
 *   A skipped AMP step counts: GradScaler's skip is decided on the device, the average counts every
 * yk_trainer_apply, so t and w_t are host-known and no step reads the device; on a skipped step p is unchanged
 * and the shadow moves once more toward the same p.
 *   yk_trainer_set(which = 0) does not touch the shadow: it is a parameter load, and the caller decides with
 * yk_trainer_ema_set. */
int yk_trainer_set_ema(yk_trainer_t* t, double decay, int every);
/* the shadow's DEVICE pointer (nparams floats, the layout of yk_trainer_buffers' params), for zero-copy views;
 * YK_ERR_STATE when the average is off */
int yk_trainer_ema_buffer(yk_trainer_t* t, float** ema);
/* the shadow to HOST arrays in state_dict order, as yk_trainer_get takes them (NULL entries skipped);
 * synchronises; YK_ERR_STATE when off */
int yk_trainer_ema_get(yk_trainer_t* t, float* const* out);
/* in: HOST arrays in state_dict order (NULL entries skipped) copied into the shadow, or in == NULL: the current
 * parameters copied into it on the device.  updates >= 0 also sets the count of updates made (and the applies
 * since the last one to 0); negative: both stay.  Synchronises; YK_ERR_STATE when off */
int yk_trainer_ema_set(yk_trainer_t* t, const float* const* in, int64_t updates);
/* HOST out[4]: decay, every, updates made, applies since the last update; all zeros when off */
int yk_trainer_ema_state(yk_trainer_t* t, double* out /* HOST [4] */);

#ifdef __cplusplus
}
#endif
#endif /* YACHT_HIP_H */
