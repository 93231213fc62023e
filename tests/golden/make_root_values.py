"""Generate tests/golden/root_values_hash.npz by running the REFERENCE's own search.

Run only where the reference lives (never on a GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_root_values.py

Re-runs the seven episodes of ``episodes_hash.npz`` (seed 20251015, envs 0-6 with their sims / cpuct /
tempThreshold) through ``make_golden.run_episode`` - the reference's Coach.executeEpisode with the RNG
entry points of make_golden replaced by the per-game stream - with ``MCTS.getActionProb`` wrapped at class
level (run_episode's own per-instance wrapper calls through to it).  After each call the wrapper dumps the
root's ``(action, Nsa, float(Qsa))`` triples in ascending action order and the root value of DESIGN.md
section 7b-val computed from them in Python floats (float64, one rounding per operation):

    num = 0.0; den = 0.0
    for each triple:  num = num + float(N) * Q ;  den = den + float(N)
    q64 = num / den

The visit counts are asserted equal to those in episodes_hash.npz.  Only data is written.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402  (patches the reference's RNG entry points on import)

from MCTS import MCTS  # noqa: E402

EPISODES = ((0, 25, 1.5, 15), (1, 25, 1.5, 15), (2, 25, 1.5, 15), (3, 8, 1.5, 15), (4, 2, 1.5, 15),
            (5, 25, 1.0, 49), (6, 100, 1.5, 15))  # (env, sims, cpuct, tempThreshold): make_golden.main's
SEED = 20251015

_ROOTS = []  # one entry per getActionProb call of the episode being played
_orig_gap = MCTS.getActionProb


def _gap(self, canonicalBoard, temp=1):
    pi = _orig_gap(self, canonicalBoard, temp=temp)
    s = self.game.stringRepresentation(canonicalBoard)
    triples = [(a, int(self.Nsa[(s, a)]), float(self.Qsa[(s, a)])) for a in range(3226) if (s, a) in self.Nsa]
    num, den = 0.0, 0.0
    for _, n, q in triples:
        if n > 0:
            num = num + float(n) * q
            den = den + float(n)
    _ROOTS.append((triples, num / den if den else float("nan")))
    return pi


def main():
    MCTS.getActionProb = _gap
    gold = np.load(os.path.join(HERE, "episodes_hash.npz"))
    acts, ns, qs = [], [], []
    E = len(EPISODES)
    nm = int(gold["moves"].shape[1])
    off = np.zeros((E, nm + 1), dtype=np.int64)
    n_moves = np.zeros(E, dtype=np.int32)
    q64 = np.full((E, nm), np.nan, dtype=np.float64)
    players = np.zeros((E, nm), dtype=np.int32)
    values = np.zeros((E, nm), dtype=np.float64)
    k = 0
    for i, (env, sims, cpuct, tt) in enumerate(EPISODES):
        assert [int(x) for x in gold["meta"][i, :4]] == [SEED, env, sims, tt] and gold["cpuct"][i] == cpuct
        del _ROOTS[:]
        ep = MG.run_episode(SEED, env, sims, cpuct, tt)
        T = len(ep["moves"])
        assert T == len(_ROOTS) == int(gold["meta"][i, 4])
        n_moves[i] = T
        for j, (triples, q) in enumerate(_ROOTS):
            a0, a1 = int(gold["count_off"][i, j]), int(gold["count_off"][i, j + 1])
            assert [t[0] for t in triples] == [int(x) for x in gold["count_action"][a0:a1]], (i, j)
            assert [t[1] for t in triples] == [int(x) for x in gold["count_n"][a0:a1]], (i, j)
            assert triples == [(a, n, qq) for (a, n), (_, _, qq) in zip(ep["moves"][j]["counts"], triples)]
            off[i, j] = k
            for a, n, qq in triples:
                acts.append(a)
                ns.append(n)
                qs.append(qq)
                k += 1
            q64[i, j] = q
            players[i, j] = ep["moves"][j]["player"]
            values[i, j] = ep["values"][j]
        off[i, T:] = k
        assert np.array_equal(values[i, :T], gold["values"][i, :T])
        print(f"episode env={env} sims={sims}: {T} moves, {k} triples so far")
    np.savez_compressed(os.path.join(HERE, "root_values_hash.npz"),
                        meta=gold["meta"][:, :5], cpuct=gold["cpuct"], n_moves=n_moves, players=players,
                        values=values, triple_off=off, triple_action=np.array(acts, dtype=np.int32),
                        triple_n=np.array(ns, dtype=np.int32), triple_q=np.array(qs, dtype=np.float64), q64=q64)


if __name__ == "__main__":
    main()
