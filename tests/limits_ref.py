"""The search past its fixed capacities ("limits"; csrc/yk_engine_dev.h RV_CAP, RO_K), on
fpu_ref's plain-Python MCTS.  TEST INFRASTRUCTURE ONLY - thin helpers, no search of its own.

  wide_root / root_of_width   rows of golden/states.npz by their number of valid actions
  search_twice                one FpuMCTS, get_action_counts twice on the same root (yk_mcts_search's persistent
                              tree), with the root's distinct visited edges after every simulation - counted
                              inside the reference by a dict that watches the insertions into Nsa
  episode                     fpu_ref.play_episode with the four counters per move
  arena_games                 plain games with the engine's arena books kept beside them (entries in use per move)
  dev_constant                a `constexpr int NAME = value;` of csrc/yk_engine_dev.h, read as text
  SIMS .. FORCED_K, search_case, game_case   the cases both test modules share
Each reference is computed once per argument tuple and shared (read-only) by the tests of a module."""
import os
import re

import numpy as np

import fpu_ref as FR
from oracle import oracle as O
from oracle import spec

ASIZE = FR.ASIZE
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DEV_H = os.path.join(os.path.dirname(HERE), "nypc-yacht-auction_amd", "csrc", "yk_engine_dev.h")
_cache = {}

# The cases of test_gpu_search_limits.py, which test_search_limits_host.py proves on the reference alone.
# cpuct 200 makes every search follow the prior (at the engine's usual 1.5 the wide root visits 41 edges).  The
# self-play game needs more simulations than the external roots: forced playouts (k = 2) send about every second
# simulation back to a visited edge, which holds a 10-dice root at ~700 distinct edges after 1300 simulations,
# ~1000 after 2000 and ~1200 after 2400 - and no cpuct changes that, a forced edge's u is +inf.
SIMS, GAME_SIMS, CPUCT = 1300, 2400, 200.0
RED, ROOT_RED = 0.25, 0.5            # first-play urgency: interior, and the external roots' own
SEARCH_SEED = 77
SEARCH_ROOTS = ((900, 3024), (901, 3024), (902, 2772), (903, 202))  # (env, the root's valid actions) per tree
GAME_SEED, GAME_ENV, GAME_MOVES, FORCED_K = 2026, 300, 6, 2.0


def search_case(r):
    """search_twice of the four trees of test (a) under r (None: first-play urgency off)."""
    return [search_twice(SEARCH_SEED, env, root_of_width(w), SIMS, CPUCT, r, None if r is None else ROOT_RED)
            for env, w in SEARCH_ROOTS]


def game_case(env=GAME_ENV):
    return episode(GAME_SEED, env, GAME_SIMS, CPUCT, RED, FORCED_K, GAME_MOVES)


def dev_constant(name):
    with open(DEV_H) as f:
        m = re.findall(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), f.read(), flags=re.M)
    assert len(m) == 1, (name, m)
    return int(m[0])


def root_of_width(width):
    """The first row of golden/states.npz with `width` valid actions for player 1 that player 1 can move from
    (uint64[8]).  The file also holds boards seen from the seat that has already bid: their 202 "valid" bids all
    raise in getNextState (YK_ST_ASSERT), which no search may start from."""
    key = ("root", width)
    if key not in _cache:
        st = np.load(os.path.join(GOLDEN, "states.npz"))["states"].astype(np.uint64)
        nv = O.valid(st, 1)[0].sum(axis=1)
        for row in np.flatnonzero(nv == width):
            a = int(np.flatnonzero(O.valid(st[row], 1)[0][0])[0])
            if int(O.step(st[row], 1, a, 0, 0, 0)[2][0]) == 0:
                break
        else:
            raise AssertionError(width)
        _cache[key] = st[int(row)].copy()
        _cache[key].setflags(write=False)
    return _cache[key]


def wide_root():
    return root_of_width(3024)


class _WatchedNsa(dict):
    """Nsa that counts the distinct edges of one state as they are inserted."""

    def __init__(self, s):
        super().__init__()
        self.s, self.n = s, 0

    def __setitem__(self, key, value):
        if key[0] == self.s and key not in self:
            self.n += 1
        super().__setitem__(key, value)


def _dense(got):
    counts = np.zeros(ASIZE, dtype=np.int32)
    for a, c in got.items():
        counts[a] = c
    return counts


def search_twice(seed, env, root, sims, cpuct, r=None, r_root=None):
    """-> dict: counts (two int32[3226]), ctr (the stream counter after each call), fpu_picks /
    fpu_unvisited_picks (the reference's sums after each call), edges (int[2 * sims]: the root's distinct visited
    edges after every simulation of both calls), max_n (the root's largest N after each call), root_p (the root's
    prior, dense)."""
    root = np.asarray(root, dtype=np.uint64)
    key = ("twice", seed, env, root.tobytes(), sims, cpuct, r, r_root)
    if key in _cache:
        return _cache[key]
    rs = spec.Stream(seed, env, 0)
    mcts = FR.FpuMCTS(seed, env, rs, 0, cpuct, r, r_root)
    mcts.Nsa = nsa = _WatchedNsa(root.tobytes())
    out = dict(counts=[], ctr=[], fpu_picks=[], fpu_unvisited_picks=[], edges=[], max_n=[])
    for _ in range(2):
        for _ in range(sims):  # get_action_counts' loop (MCTS.py:37-38), with the watch read between its searches
            mcts.search(root)
            out["edges"].append(nsa.n)
        got = mcts.get_action_counts(root)  # (sims = 0: the root's counts as they stand)
        assert nsa.n == len(got)
        out["counts"].append(_dense(got))
        out["ctr"].append(rs.ctr)
        out["fpu_picks"].append(mcts.fpu_picks)
        out["fpu_unvisited_picks"].append(mcts.fpu_unvisited_picks)
        out["max_n"].append(max(got.values()))
    out["root_p"] = mcts.Ps[root.tobytes()].copy()  # float32[3226], 0 off the valid set
    for c in out["counts"] + [out["root_p"]]:
        c.setflags(write=False)
    _cache[key] = out
    return out


def first_above(edges, cap):
    """The 0-based simulation after which `edges` first exceeds cap (None: never)."""
    hit = np.flatnonzero(np.asarray(edges) > cap)
    return int(hit[0]) if len(hit) else None


class _PerMove(FR.FpuMCTS):
    """FpuMCTS that notes its counters after every get_action_counts (one per move of play_episode)."""

    def get_action_counts(self, board, root_prior=None):
        got = super().get_action_counts(board, root_prior)
        self.__dict__.setdefault("marks", []).append((self.forced_picks, self.fpu_picks, self.fpu_unvisited_picks))
        return got


class _ArenaModel(FR.FpuMCTS):
    """FpuMCTS that keeps the engine's arena books: a node takes its valid count rounded up to
    4 entries; a move whose root is of a later round than the tree's first drops the nodes of earlier rounds
    (k_move_begin's compaction).  `tops`: the entries in use after each move's search - within a move they only grow."""

    def get_action_counts(self, board, root_prior=None):
        bk = self.__dict__.setdefault("books", dict(live=[], seen=0, round=0))
        tops = self.__dict__.setdefault("tops", [])
        rr = int(board[0]) & 0xF
        if rr > bk["round"]:
            bk["live"] = [n for n in bk["live"] if n[0] >= rr]
            bk["round"] = rr
        got = super().get_action_counts(board, root_prior)
        keys = list(self.Ps)  # (insertion order: the expansions in theirs)
        for s in keys[bk["seen"]:]:
            bk["live"].append((int(np.frombuffer(s, dtype=np.uint64)[0]) & 0xF, (int(np.count_nonzero(self.Vs[s])) + 3) & ~3))
        bk["seen"] = len(keys)
        tops.append(sum(vp for _, vp in bk["live"]))
        return got


def arena_games(seed, envs, sims, cpuct, max_moves=48):
    """Plain games (no opt-in feature) with the arena's books -> [(play_episode's dict, tops per move)]."""
    key = ("arena", seed, tuple(envs), sims, cpuct, max_moves)
    if key not in _cache:
        out = []
        for env in envs:
            made = []

            def make(*a):
                made.append(_ArenaModel(*a))
                return made[-1]

            g = FR.play_episode(seed, env, sims, cpuct=cpuct, max_moves=max_moves, mcts_class=make)
            out.append((g, list(made[0].tops)))
        _cache[key] = out
    return _cache[key]


def episode(seed, env, sims, cpuct, r, k, max_moves):
    """fpu_ref.play_episode(seed, env, sims, r=r, k=k, cpuct=cpuct, max_moves=max_moves) plus `per_move`: for each
    move a dict of forced_picks, pruned_visits, fpu_picks, fpu_unvisited_picks (that move's own) and raw_edges."""
    key = ("episode", seed, env, sims, cpuct, r, k, max_moves)
    if key in _cache:
        return _cache[key]
    made = []

    def make(*a):
        made.append(_PerMove(*a))
        return made[-1]

    g = FR.play_episode(seed, env, sims, r=r, k=k, cpuct=cpuct, max_moves=max_moves, mcts_class=make)
    marks = [(0, 0, 0)] + made[0].marks
    g["per_move"] = [dict(forced_picks=marks[m + 1][0] - marks[m][0], fpu_picks=marks[m + 1][1] - marks[m][1],
                          fpu_unvisited_picks=marks[m + 1][2] - marks[m][2],
                          pruned_visits=sum(g["raw"][m].values()) - sum(g["kept"][m].values()),
                          raw_edges=len(g["raw"][m])) for m in range(g["n_moves"])]
    _cache[key] = g
    return g
