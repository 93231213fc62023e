"""The self-play temperatures restated (include/yacht_hip.h, yk_engine_set_temperatures /
yk_temperature_schedule / yk_temperature_pick / yk_root_temper).  TEST INFRASTRUCTURE ONLY.

Plain Python floats (float64) and the host libm's pow (Python's ``**`` on floats):
  schedule(early, final, halflife, n)   T(m) = final + (early - final) * 2.0 ** (-m / halflife), m = 0 .. n-1
  pick(counts, T, u)                    w_i = float(n_i) ** (1.0 / T); total = the left-to-right sum of w_i;
                                        c_i = c_(i-1) + w_i / total; last = c_(n-1); the first i with c_i / last > u
                                        -> (i, total, margin), margin = min_i |c_i / last - u|
  root_temper(P, T)                     w_j = float(P_j) ** (1.0 / T); S = the left-to-right sum of w_j;
                                        P'_j = float32(w_j / S); T == 1.0 exactly (or S not > 0): P itself
on top of noise_ref's Coach / MCTS (forced_ref's when forced playouts are on): play_episode draws every temp-1
move through pick with the move schedule's T(m), and replaces each real move's root prior by root_temper under the
root schedule's T(m) - or by whatever the `root_prior` callback returns - at the top of getActionProb."""
import numpy as np

import forced_ref as F
import noise_ref as R
from oracle import oracle as O
from oracle import spec

ASIZE = R.ASIZE
MOVE_RANGE = (0.05, 100.0)
ROOT_RANGE = (0.25, 10.0)

# The games tests/test_gpu_temper.py replays through play_episode and demands exact actions of.  The device's pow
# and libm's differ by ulps, so each of them must keep the reference itself away from a draw boundary:
# tests/test_temper_host.py checks, on the CPU, that every one has a draw margin >= MARGIN.
MARGIN = 1e-9
SEED, ENV_BASE, N_GAMES, SIMS = 11, 3, 2, 6
MOVE_SCHEDULE = dict(early=1.3, final=0.3, halflife=8.0)    # (KataGo's shape; the values are the tests')
ROOT_SCHEDULE = dict(early=1.25, final=1.1, halflife=8.0)   # KataGo's root policy temperatures
THRESHOLDS = (49, 15)  # tempThreshold: a draw at every move, and the reference's default


# ------------------------------------------------------------------ the definitions (normative)
def schedule(early, final, halflife, n_moves):
    if early == final:  # (a flat schedule needs no halflife)
        return np.full(n_moves, float(final), dtype=np.float64)
    return np.array([final + (early - final) * 2.0 ** (-m / halflife) for m in range(n_moves)], dtype=np.float64)


def pick(counts, T, u):
    """-> (index within the row or -1, total, margin)."""
    w = [float(int(n)) ** (1.0 / T) for n in counts]
    total = 0.0
    for x in w:
        total += x
    if not total > 0.0:
        return -1, total, float("inf")
    cdf, c = [], 0.0
    for x in w:
        c += x / total
        cdf.append(c)
    last = cdf[-1]
    got = next((i for i, c in enumerate(cdf) if c / last > u), -1)
    return got, total, min(abs(c / last - u) for c in cdf)


def root_temper(P, T):
    """P: float32 vector (compact, or dense with zeros off the valid set: a zero adds nothing to S and stays 0)."""
    P = np.asarray(P, dtype=np.float32)
    if T == 1.0:
        return P.copy()
    w = [float(p) ** (1.0 / T) for p in P]
    S = 0.0
    for x in w:
        S += x
    if not S > 0.0:
        return P.copy()
    return np.array([x / S for x in w], dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------ Coach / MCTS in plain Python
def play_episode(seed, env, sims, move_t=None, root_t=None, cpuct=1.5, temp_threshold=15, max_moves=48,
                 root_prior=None, k=0.0, prune=True):
    """noise_ref.play_episode (forced_ref's with k > 0) under the two schedules: move_t / root_t are tables of T by
    real move (schedule(...)) or None for off.  root_prior(move, Ps) -> the root's new Ps replaces the default -
    root_temper under root_t[move] - when given (the GPU tests hand the device's own prior back).  Returns the
    record fields plus `margin`, the smallest |c_i / last - u| met by any temp-1 draw of the game."""
    board, ctr = O.init_board(seed, [env])
    board, rs = board[0], spec.Stream(seed, env, int(ctr[0]))
    mcts = F.ForcedMCTS(seed, env, rs, sims, cpuct) if k > 0 else R.PyMCTS(seed, env, rs, sims, cpuct)
    if root_prior is None and root_t is not None:
        root_prior = lambda move, P: root_temper(P, float(root_t[move]))  # noqa: E731
    cur, step = 1, 0
    states, info, ctrs, visits, voff = [], [], [], [], [0]
    margin = float("inf")
    while True:
        step += 1
        move = step - 1
        canon = O.canonical(board, cur)[0]
        temp = int(step < temp_threshold)
        c0 = rs.ctr
        if k > 0:
            mcts.k = float(k)
        counts = mcts.get_action_counts(canon, None if root_prior is None else (lambda P: root_prior(move, P)))
        s = canon.tobytes()
        root_ns = mcts.Ns.get(s, -1)
        acts = sorted(counts)
        n = [counts[a] for a in acts]
        if k > 0 and prune and acts:
            got = F.prune_row(acts, n, [mcts.Qsa[(s, a)] for a in acts], [mcts.Ps[s][a] for a in acts], root_ns, k, cpuct)
            acts, n = [a for a, c in zip(acts, got) if c > 0], [c for c in got if c > 0]
        if temp == 0:  # MCTS.py:44-49, then Coach.py:65's draw over the one-hot pi: untouched by the temperatures
            mx = max(n) if n else 0
            if mx == 0:
                action = rs.below(ASIZE)
            else:
                best = [a for a, c in zip(acts, n) if c == mx]
                action = best[rs.below(len(best))]
            rs.uniform53()
        else:  # one uniform whatever T; T = 1.0 is the reference's own draw (n ** 1.0 == n)
            T = 1.0 if move_t is None else float(move_t[move])
            u = rs.uniform53()
            i, _, mg = pick(n, T, u)
            margin = min(margin, mg)
            action = acts[i]
        states.append(canon)
        info.append([temp, cur, action, mcts.expansions, root_ns, len(acts), 0, 0])
        ctrs.append([c0, rs.ctr])
        visits += [[a, c] for a, c in zip(acts, n)]
        voff.append(len(visits))
        nxt, npl, st, ctr = O.step(board, cur, action, seed, env, rs.ctr)
        assert st[0] == 0
        rs.ctr = int(ctr[0])
        board, cur = nxt[0], int(npl[0])
        r = float(O.ended(board, cur)[0][0])
        if r != 0 or step >= max_moves:
            break
    players = np.array([i[1] for i in info])
    return dict(states=np.array(states, dtype=np.uint64), info=np.array(info, dtype=np.int32),
                ctr=np.array(ctrs, dtype=np.uint64), values=r * np.where(players != cur, -1.0, 1.0),
                final=board.astype(np.uint64), n_moves=step, visits=np.array(visits, dtype=np.int32).reshape(-1, 2),
                visits_off=np.array(voff, dtype=np.int64), margin=margin)
