"""Forced playouts and policy target pruning restated (include/yacht_hip.h,
yk_engine_set_forced_playouts / yk_policy_prune).  TEST INFRASTRUCTURE ONLY.

The rule in plain Python floats (every quantity a float64; P is the float32 the search holds, converted):
  forced(N, P, Ns, k)      N > 0 and N * N < (k * P) * Ns                      - the edge's u is +inf
  prune_row(...)           c* = largest N, lowest action among equals, keeps N; PUCT* = Q* + (c P*) sqrt(Ns) / (1 + N*);
                           every other visited edge: f = the largest integer with f * f <= (k P) Ns; from n = N,
                           n -= 1 while n > 0, N - n < f and Q + (c P) sqrt(Ns) / (1 + (n - 1)) < PUCT*; an n
                           brought to exactly 1 becomes 0
on top of noise_ref's Coach / MCTS: ForcedMCTS applies the forced test at depth 0 of a real move's search, and
play_episode prunes the move's counts before it records them and draws the move from them."""
import math

import numpy as np

import noise_ref as R
from oracle import oracle as O
from oracle import spec

ASIZE = R.ASIZE
REC_FAST = 0x100


# ------------------------------------------------------------------ the rule (normative)
def forced(N, P, Ns, k):
    return N > 0 and float(N) * float(N) < (k * float(P)) * float(Ns)


def floor_root(x):
    """The largest integer f with float(f) * float(f) <= x (0 when there is none)."""
    if not x > 0.0:
        return 0
    f = int(math.sqrt(x))
    while float(f + 1) * float(f + 1) <= x:
        f += 1
    while f > 0 and float(f) * float(f) > x:
        f -= 1
    return f


def puct(Q, P, Ns, c, n):
    return float(Q) + (c * float(P)) * math.sqrt(float(Ns)) / (1 + n)


def prune_row(acts, N, Q, P, Ns, k, c):
    """Pruned counts of one root: acts (the tie rule: the lowest wins), N, Q, P per visited edge (N > 0)."""
    if not len(N):
        return []
    k, c = float(k), float(c)
    best = max(N)
    star = min((a, i) for i, a in enumerate(acts) if N[i] == best)[1]
    bound = puct(Q[star], P[star], Ns, c, N[star])
    out = []
    for i in range(len(N)):
        n = int(N[i])
        if i != star:
            f = floor_root((k * float(P[i])) * float(Ns))
            while n > 0 and N[i] - n < f and puct(Q[i], P[i], Ns, c, n - 1) < bound:
                n -= 1
            if n == 1 and n < N[i]:
                n = 0
        out.append(n)
    return out


def policy_prune(indptr, cols, counts, q, p, ns, k, cpuct):
    """yk_policy_prune in numpy: rows of a CSR -> the pruned counts (int32).  Entries with counts <= 0 are no
    visited edges and keep their word."""
    counts = np.asarray(counts, dtype=np.int32)
    out = counts.copy()
    for r in range(len(indptr) - 1):
        a, b = int(indptr[r]), int(indptr[r + 1])
        vis = [i for i in range(a, b) if counts[i] > 0]
        got = prune_row([int(cols[i]) for i in vis], [int(counts[i]) for i in vis], [float(q[i]) for i in vis],
                        [p[i] for i in vis], max(int(ns[r]), 0), k, cpuct)
        for i, n in zip(vis, got):
            out[i] = n
    return out


# ------------------------------------------------------------------ Coach / MCTS in plain Python
class ForcedMCTS(R.PyMCTS):
    """noise_ref.PyMCTS whose search applies the forced test at depth 0 while `self.k` > 0 (play_episode sets it
    for the searches of a full move and clears it for a fast one)."""

    def __init__(self, seed, env, stream, sims, cpuct):
        super().__init__(seed, env, stream, sims, cpuct)
        self.k = 0.0
        self.forced_picks = 0

    def search(self, board, depth=0):  # noise_ref.PyMCTS.search with `depth` and the forced test
        s = board.tobytes()
        if s not in self.Es:
            self.Es[s] = float(O.ended(board, 1)[0][0])
        if self.Es[s] != 0:
            return -self.Es[s]
        if s not in self.Ps:
            pi, v = O.hash_prior(board)
            valids = O.valid(board, 1)[0][0].astype(np.float32)
            P = pi[0] * valids
            sum_Ps_s = np.sum(P)
            if sum_Ps_s > 0:
                P /= sum_Ps_s
            else:
                P = P + valids
                if np.sum(P) > 0:
                    P /= np.sum(P)
                else:
                    P = np.zeros(ASIZE, dtype=np.float32)
                    P[0] = 1.0
            self.Ps[s], self.Vs[s], self.Ns[s] = P, valids, 0
            self.expansions += 1
            return -v[0]
        valids = self.Vs[s]
        P = self.Ps[s]
        u = (np.float32(self.cpuct) * P) * np.float32(math.sqrt(self.Ns[s] + R.EPS))
        u = np.where(valids > 0, u, -np.inf).astype(np.float64)
        for a in np.flatnonzero(valids):
            a = int(a)
            if (s, a) in self.Qsa:
                u[a] = self.Qsa[(s, a)] + self.cpuct * P[a] * math.sqrt(self.Ns[s]) / (1 + self.Nsa[(s, a)])
                if depth == 0 and self.k > 0 and forced(self.Nsa[(s, a)], P[a], self.Ns[s], self.k):
                    u[a] = np.inf
        a = int(np.argmax(u)) if u.size and np.max(u) > -np.inf else -1
        if a == -1 or not valids[a]:
            va = np.flatnonzero(valids == 1)
            if len(va) == 0:
                return 0
            a = int(va[0])
        elif depth == 0 and u[a] == np.inf:
            self.forced_picks += 1
        nxt, npl, st, ctr = O.step(board, 1, a, self.seed, self.env, self.rs.ctr)
        assert st[0] == 0
        self.rs.ctr = int(ctr[0])
        v = self.search(O.canonical(nxt, npl)[0], depth + 1)
        if (s, a) in self.Qsa:
            self.Qsa[(s, a)] = (self.Nsa[(s, a)] * self.Qsa[(s, a)] + v) / (self.Nsa[(s, a)] + 1)
            self.Nsa[(s, a)] += 1
        else:
            self.Qsa[(s, a)] = v
            self.Nsa[(s, a)] = 1
        self.Ns[s] += 1
        return -v


def play_episode(seed, env, sims, k, prune=True, cpuct=1.5, temp_threshold=15, max_moves=48, root_prior=None,
                 full=None, fast_sims=0):
    """noise_ref.play_episode with forced playouts (k) and, with `prune`, the pruned counts recorded and drawn
    from.  full (bool per move, None: every move) / fast_sims: the playout cap's schedule - a fast move runs
    fast_sims simulations without noise, forcing or pruning, and its status word carries REC_FAST.  Returns the
    record fields plus forced_picks, pruned_visits, and per move `raw` (the unpruned {action: N}) and `kept`."""
    board, ctr = O.init_board(seed, [env])
    board, rs = board[0], spec.Stream(seed, env, int(ctr[0]))
    mcts = ForcedMCTS(seed, env, rs, sims, cpuct)
    cur, step = 1, 0
    states, info, ctrs, visits, voff, raws, kept = [], [], [], [], [0], [], []
    pruned_visits = 0
    while True:
        step += 1
        move = step - 1
        is_full = full is None or bool(full[move])
        canon = O.canonical(board, cur)[0]
        temp = int(step < temp_threshold)
        c0 = rs.ctr
        mcts.sims = sims if is_full else fast_sims
        mcts.k = float(k) if is_full else 0.0
        counts = mcts.get_action_counts(
            canon, None if root_prior is None or not is_full else (lambda P: root_prior(move, P)))
        s = canon.tobytes()
        root_ns = mcts.Ns.get(s, -1)
        acts = sorted(counts)
        n = [counts[a] for a in acts]
        raws.append(dict(counts))
        if is_full and k > 0 and prune and acts:
            got = prune_row(acts, n, [mcts.Qsa[(s, a)] for a in acts], [mcts.Ps[s][a] for a in acts], root_ns, k, cpuct)
            pruned_visits += sum(n) - sum(got)
            acts, n = [a for a, c in zip(acts, got) if c > 0], [c for c in got if c > 0]
        kept.append(dict(zip(acts, n)))
        if temp == 0:
            mx = max(n) if n else 0
            if mx == 0:
                action = rs.below(ASIZE)
            else:
                best = [a for a, c in zip(acts, n) if c == mx]
                action = best[rs.below(len(best))]
            rs.uniform53()
        else:
            total = float(sum(n))
            cdf, c = [], 0.0
            for x in n:
                c += x / total
                cdf.append(c)
            u = rs.uniform53()
            action = next(a for a, c in zip(acts, cdf) if c / cdf[-1] > u)
        states.append(canon)
        info.append([temp, cur, action, mcts.expansions, root_ns, len(acts), 0 if is_full else REC_FAST, 0])
        ctrs.append([c0, rs.ctr])
        visits += [[a, c] for a, c in zip(acts, n)]
        voff.append(len(visits))
        nxt, npl, st, ctr = O.step(board, cur, action, seed, env, rs.ctr)
        assert st[0] == 0
        rs.ctr = int(ctr[0])
        board, player, cur = nxt[0], cur, int(npl[0])
        info[-1][1] = player
        r = float(O.ended(board, cur)[0][0])
        if r != 0 or step >= max_moves:
            break
    players = np.array([i[1] for i in info])
    return dict(states=np.array(states, dtype=np.uint64), info=np.array(info, dtype=np.int32),
                ctr=np.array(ctrs, dtype=np.uint64), values=r * np.where(players != cur, -1.0, 1.0),
                final=board.astype(np.uint64), n_moves=step, visits=np.array(visits, dtype=np.int32).reshape(-1, 2),
                visits_off=np.array(voff, dtype=np.int64), forced_picks=mcts.forced_picks,
                pruned_visits=pruned_visits, raw=raws, kept=kept)
