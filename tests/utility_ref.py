"""The score-margin utility restated (include/yacht_hip.h, yk_engine_set_score_utility /
yk_score_utility / yk_examples_utility_targets).  TEST INFRASTRUCTURE ONLY.

The rule in numpy float64, one operation per line, each rounded on its own: for a terminal state s seen from
`player` (+1 / -1), weight w in [0, 1] and scale c > 0 (game points),
    z = getGameEnded(s, player)                          (+-1; 1e-4 for a draw, for either player)
    m = total_with_bonus(p1) - total_with_bonus(p2)      (int)
    x = float64(player * m) / c
    g = x / (1 + |x|)
    u = (1 - w) * z + w * g
on top of fpu_ref's Coach / MCTS: UtilityMCTS returns -u(s, 1) where the reference's search returns -Es, counts
those returns, and notes each move's root-value word; play_episode is fpu_ref's with it; value_targets is
value_ref's with U_t = (1 - w) Z_t + w g1 read for Z_t."""
import numpy as np

import fpu_ref as FR
import value_ref as V
from oracle import oracle as O
from oracle import spec

ASIZE = FR.ASIZE
ONE = np.float64(1.0)


# ------------------------------------------------------------------ the rule (normative)
def margin(state):
    """m of a state: player 1's total with bonus less player 2's (a Python int)."""
    tot = O.ended(np.asarray(state, dtype=np.uint64), 1)[1][0]
    return int(tot[0]) - int(tot[1])


def squash(player, m, c):
    """g for `player` from the margin m."""
    x = np.float64(int(player) * int(m)) / np.float64(c)
    return x / (ONE + np.abs(x))


def blend(z, g, w):
    keep = ONE - np.float64(w)
    return keep * np.float64(z) + np.float64(w) * np.float64(g)


def utility(final_or_state, player, w, c):
    """u of a state seen from `player` as a numpy float64; 0.0 for a state that is not terminal."""
    state = np.asarray(final_or_state, dtype=np.uint64)
    z = np.float64(O.ended(state, int(player))[0][0])
    if z == 0:
        return np.float64(0.0)
    return blend(z, squash(player, margin(state), c), w)


# ------------------------------------------------------------------ Coach / MCTS in plain Python
class UtilityMCTS(FR.FpuMCTS):
    """fpu_ref.FpuMCTS whose terminal value is the rule while `self.w` is not None (a Python float, as the
    reference's -Es is).  `terminal_returns` counts the searches that ended at a terminal state, on or off;
    `terminals` keeps the distinct terminal states' margins; `root_words` gets, after every get_action_counts
    (one per move of play_episode), the move's root-value word (value_ref.root_value / encode of the root's
    (action, N, Q) triples)."""
    w = None
    c = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.terminal_returns = 0
        self.terminals = {}
        self.root_words = []

    def search(self, board, depth=0):
        s = board.tobytes()
        if s not in self.Es:
            self.Es[s] = float(O.ended(board, 1)[0][0])
        if self.Es[s] != 0:  # terminal: Es decides, never u (at w = 1 a draw has u = 0)
            self.terminal_returns += 1
            self.terminals[s] = margin(board)
            if self.w is None:
                return -self.Es[s]
            return -float(utility(board, 1, self.w, self.c))
        return super().search(board, depth)

    def get_action_counts(self, board, root_prior=None):
        got = super().get_action_counts(board, root_prior)
        s = board.tobytes()
        triples = [(a, int(self.Nsa[(s, a)]), float(self.Qsa[(s, a)])) for a in range(ASIZE) if (s, a) in self.Nsa]
        with np.errstate(invalid="ignore"):
            self.root_words.append(int(V.encode(np.float32(V.root_value(triples)))) if triples else 0)
        return got


def mcts_class(w=None, c=None):
    """UtilityMCTS with the knobs bound (fpu_ref.play_episode and arena_game build their searches themselves)."""
    return type("UtilityMCTS_%s_%s" % (w, c), (UtilityMCTS,), dict(w=w, c=c))


def play_episode(seed, env, sims, w=None, c=None, root_values=True, **kw):
    """fpu_ref.play_episode with the utility (w, c; None: off) in every search of the game.  Returns its dict
    plus root_words (uint32[n_moves]: each move's root-value word; with root_values they are also info[:, 7], as
    an engine with record_root_values records them), terminal_returns and margins (the distinct terminal states'
    margins)."""
    made = []
    cls = mcts_class(w, c)

    def make(*a):
        made.append(cls(*a))
        return made[0]
    g = FR.play_episode(seed, env, sims, mcts_class=make, **kw)
    m = made[0]
    words = np.array(m.root_words, dtype=np.uint32)
    assert len(words) == g["n_moves"]
    if root_values:
        g["info"][:, 7] = words.view(np.int32)
    g.update(root_words=words, terminal_returns=m.terminal_returns, margins=sorted(m.terminals.values()))
    return g


def search_counts(seed, env, root, sims, cpuct, w=None, c=None, ctr=0, **kw):
    """yk_mcts_search of one external root on a fresh tree -> (counts int32[3226], the stream counter after,
    the UtilityMCTS)."""
    rs = spec.Stream(seed, env, int(ctr))
    mcts = mcts_class(w, c)(seed, env, rs, sims, cpuct, **kw)
    got = mcts.get_action_counts(np.asarray(root, dtype=np.uint64))
    counts = np.zeros(ASIZE, dtype=np.int32)
    for a, n in got.items():
        counts[a] = n
    return counts, rs.ctr, mcts


def arena_game(seed, env, seat, sims, w=None, c=None, **kw):
    """fpu_ref.arena_game played with UtilityMCTS (both players of opponent="mcts"); the result and totals it
    returns are the game's own."""
    cls = mcts_class(w, c)
    made = []

    class Spy(cls):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    saved = FR.FpuMCTS
    FR.FpuMCTS = Spy
    try:
        g = FR.arena_game(seed, env, seat, sims, **kw)
    finally:
        FR.FpuMCTS = saved
    g["terminal_returns"] = sum(m.terminal_returns for m in made)
    return g


# ------------------------------------------------------------------ the value targets
def value_targets(q, z, players, n_moves, beta, lam, g1, w):
    """value_ref.value_targets with U_t = (1 - w) * Z_t + w * g1 for Z_t: one game, g1 the squashed final margin
    for player 1 -> float32[T]."""
    T = int(n_moves)
    beta, lam = np.float64(beta), np.float64(lam)
    keep = ONE - np.float64(w)
    p = [np.float64(int(players[t])) for t in range(T)]
    qd = [np.float64(np.float32(q[t])) for t in range(T)]
    W = [p[t] * qd[t] for t in range(T)]
    Z = [p[t] * np.float64(z[t]) for t in range(T)]
    U = [keep * Z[t] + np.float64(w) * np.float64(g1) for t in range(T)]
    G = list(U)
    if lam != 1.0:
        for t in range(T - 2, -1, -1):
            G[t] = (ONE - lam) * W[t + 1] + lam * G[t + 1]
    out = np.zeros(T, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            target = p[t] * G[t]
            v = target if beta == 0.0 else (ONE - beta) * target + beta * qd[t]
            out[t] = np.float32(v)
    return out
