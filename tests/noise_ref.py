"""Reference restatements for the Dirichlet root noise.  TEST INFRASTRUCTURE ONLY.

1. The sampler: eta ~ Dir(alpha) for (seed, env, move, V, alpha), Philox4x32-10 as in oracle/spec.py and
   float64 throughout - the normative definition yk_dirichlet_noise and the engine implement.
2. Coach.executeEpisode (Coach.py:55-72) over MCTS.getActionProb / MCTS.search (MCTS.py:28-164) in plain
   Python: dicts keyed by the packed canonical state over the oracle's game functions, NumPy float32
   priors and Python-typed values as the reference holds them (numpy 2 promotion does the rest), the
   draw rules of DESIGN.md section 5 on the game's spec.Stream - with one addition, `root_prior`: a
   callback that may replace the root's Ps once per real move, at the top of getActionProb.
"""
import math

import numpy as np

from oracle import oracle as O
from oracle import spec

M32 = spec.M32
ASIZE = spec.ACTION_SIZE
EPS = 1e-8


# ------------------------------------------------------------------ the sampler (normative)
def u53(seed, env, move, j, i):  # the game stream uses counter word 3 = 0; noise uses 0x80000000 | move
    x0, x1, _, _ = spec.philox4x32_10(i & M32, j, env & M32, 0x80000000 | move, seed & M32, (seed >> 32) & M32)
    return (((x0 | (x1 << 32)) >> 11) + 0.5) * 2.0 ** -53  # in (0, 1)


def gamma(seed, env, move, j, alpha):  # Marsaglia-Tsang; alpha < 1 boosted by u ** (1 / alpha)
    a = alpha + 1.0 if alpha < 1.0 else alpha
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    i = 0
    while True:
        u1, u2, u3 = (u53(seed, env, move, j, i + k) for k in range(3))
        i += 3
        x = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
        t = 1.0 + c * x
        if t <= 0.0:
            continue
        v = t * t * t
        if math.log(u3) < 0.5 * x * x + d - d * v + d * math.log(v):
            g = d * v
            break
    if alpha < 1.0:
        g *= u53(seed, env, move, j, i) ** (1.0 / alpha)
    return g


def eta(seed, env, move, V, alpha):
    g = [gamma(seed, env, move, j, alpha) for j in range(V)]
    s = sum(g)
    return np.array([x / s for x in g] if s > 0 else [1.0 / V] * V, dtype=np.float64)


def mix(before, eps, eta_dense):
    """P' = float32((1 - eps) * (double)P + eps * eta), in f64 and rounded once."""
    return ((1.0 - eps) * np.asarray(before, dtype=np.float64) + eps * np.asarray(eta_dense, dtype=np.float64)).astype(
        np.float32)


# ------------------------------------------------------------------ Coach / MCTS in plain Python
class PyMCTS:
    """MCTS.py:11-164 with the hash prior as nnet.predict; one instance per episode (Coach.py:93)."""

    def __init__(self, seed, env, stream, sims, cpuct):
        self.seed, self.env, self.rs, self.sims, self.cpuct = seed, env, stream, sims, cpuct
        self.Qsa, self.Nsa, self.Ns, self.Ps, self.Es, self.Vs = {}, {}, {}, {}, {}, {}
        self.expansions = 0

    def get_action_counts(self, board, root_prior=None):
        """The simulations of getActionProb (MCTS.py:37-42) -> {action: Nsa} of the root.  root_prior(Ps)
        -> the root's new Ps, applied once: before the first search when the root is in the tree, else
        right after the first search, which only expanded the root and returned (MCTS.py:84-115)."""
        s = board.tobytes()
        first = 0
        if root_prior is not None:
            if s not in self.Ps:
                self.search(board)
                first = 1
            self.Ps[s] = root_prior(self.Ps[s])
        for _ in range(first, self.sims):
            self.search(board)
        return {a: self.Nsa[(s, a)] for a in range(ASIZE) if (s, a) in self.Nsa}

    def search(self, board):
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
            else:  # (the hash prior is positive everywhere: only a node without valid moves gets here)
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
        # u over the whole action vector at once: unvisited edges cpuct * P * sqrt(Ns + EPS), visited ones
        # Q + cpuct * P * sqrt(Ns) / (1 + Nsa), each in the reference's own scalar types; strict '>' in
        # ascending action order = the first maximum
        P = self.Ps[s]
        u = (np.float32(self.cpuct) * P) * np.float32(math.sqrt(self.Ns[s] + EPS))
        u = np.where(valids > 0, u, -np.inf).astype(np.float64)
        for a in np.flatnonzero(valids):
            a = int(a)
            if (s, a) in self.Qsa:
                u[a] = self.Qsa[(s, a)] + self.cpuct * P[a] * math.sqrt(self.Ns[s]) / (1 + self.Nsa[(s, a)])
        a = int(np.argmax(u)) if u.size and np.max(u) > -np.inf else -1
        if a == -1 or not valids[a]:
            va = np.flatnonzero(valids == 1)
            if len(va) == 0:
                return 0
            a = int(va[0])
        nxt, npl, st, ctr = O.step(board, 1, a, self.seed, self.env, self.rs.ctr)
        assert st[0] == 0
        self.rs.ctr = int(ctr[0])
        v = self.search(O.canonical(nxt, npl)[0])
        if (s, a) in self.Qsa:
            self.Qsa[(s, a)] = (self.Nsa[(s, a)] * self.Qsa[(s, a)] + v) / (self.Nsa[(s, a)] + 1)
            self.Nsa[(s, a)] += 1
        else:
            self.Qsa[(s, a)] = v
            self.Nsa[(s, a)] = 1
        self.Ns[s] += 1
        return -v


def play_episode(seed, env, sims, cpuct=1.5, temp_threshold=15, max_moves=48, root_prior=None):
    """Coach.executeEpisode for one game -> the engine's record fields of that game.  root_prior(move, Ps)
    -> the root's new Ps for real move `move` (None: no noise)."""
    board, ctr = O.init_board(seed, [env])
    board, rs = board[0], spec.Stream(seed, env, int(ctr[0]))
    mcts = PyMCTS(seed, env, rs, sims, cpuct)
    cur, step = 1, 0
    states, info, ctrs, visits, voff = [], [], [], [], [0]
    while True:
        step += 1
        move = step - 1
        canon = O.canonical(board, cur)[0]
        temp = int(step < temp_threshold)
        c0 = rs.ctr
        counts = mcts.get_action_counts(canon, None if root_prior is None else (lambda P: root_prior(move, P)))
        acts = sorted(counts)
        n = [counts[a] for a in acts]
        if temp == 0:  # MCTS.py:44-49, then Coach.py:65's draw over the one-hot pi
            mx = max(n) if n else 0
            if mx == 0:
                action = rs.below(ASIZE)
            else:
                best = [a for a, c in zip(acts, n) if c == mx]
                action = best[rs.below(len(best))]
            rs.uniform53()
        else:  # MCTS.py:51-54, Coach.py:65: cumsum, /= cdf[-1], searchsorted(u, 'right')
            total = float(sum(n))
            cdf, c = [], 0.0
            for x in n:
                c += x / total
                cdf.append(c)
            u = rs.uniform53()
            action = next(a for a, c in zip(acts, cdf) if c / cdf[-1] > u)
        states.append(canon)
        info.append([temp, cur, action, mcts.expansions, mcts.Ns.get(canon.tobytes(), -1), len(acts), 0, 0])
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
                visits_off=np.array(voff, dtype=np.int64))


def assert_game_equals_records(game, rec, e, max_moves=48):
    """One play_episode result against game e of SelfPlayEngine.records(): every field, exactly."""
    M = max_moves
    n = game["n_moves"]
    assert int(rec["n_moves"][e]) == n
    assert np.array_equal(rec["states"][e, :n], game["states"])
    assert np.array_equal(rec["info"][e, :n], game["info"]), np.flatnonzero((rec["info"][e, :n] != game["info"]).any(1))
    assert np.array_equal(rec["ctr"][e, :n], game["ctr"])
    assert np.array_equal(rec["values"][e, :n], game["values"])
    assert np.array_equal(rec["final"][e], game["final"])
    off = rec["visits_off"][e * M: e * M + n + 1]
    assert np.array_equal(off - off[0], game["visits_off"])
    assert np.array_equal(rec["visits"][int(off[0]):int(off[-1])], game["visits"])
