"""Diagnostic (CPU only, reference only): how wide the root's search is under the reference rule and under
first-play urgency once the value has a consistent sign.

tests/fpu_ref.py's plain-Python Coach / MCTS plays `--games` games of `--sims` simulations with the hash prior
for P and, in place of a trained net's value, the stand-in
    v = 0.8 tanh((mover's total - opponent's total) / 30) + 0.2 v_hash
(totals with bonus, in the game's points).  Per real move it takes the number of distinct root children and the
largest child count, and reports their median (and 90th percentile) over the moves whose mover is behind, or
ahead, by `--margin` points or more.  The stand-in is not a trained net: the figures show the mechanism of the
formula, nothing about training.  Too slow for a test.

    python tools/fpu_spread.py [--games 3] [--sims 100] [--cpuct 1.0] [--r 0.3] [--margin 10] [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=3)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--cpuct", type=float, default=1.0)
    ap.add_argument("--r", type=float, default=0.3)
    ap.add_argument("--margin", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--env", type=int, default=300)
    ap.add_argument("--unit", type=float, default=1000.0, help="stored total units per point")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import fpu_ref as FR
    from oracle import oracle as O

    def margin(board):  # the mover's lead in points (a canonical board: the mover is player 1)
        tot = O.ended(board, 1)[1][0]
        return (float(tot[0]) - float(tot[1])) / a.unit

    class StandIn(FR.FpuMCTS):
        def leaf_value(self, board, v):
            return 0.8 * math.tanh(margin(board) / 30.0) + 0.2 * float(v)

    res = {"config": vars(a), "value": "0.8 tanh((mover's total - opponent's total) / 30) + 0.2 v_hash: a stand-in, "
                                       "not a trained net", "rules": {}}
    for name, r in (("reference", None), ("fpu", a.r)):
        rows = {"behind": [], "ahead": []}
        for g in range(a.games):
            ep = FR.play_episode(a.seed, a.env + g, a.sims, r=r, cpuct=a.cpuct, mcts_class=StandIn)
            for m in range(ep["n_moves"]):
                lead, raw = margin(ep["states"][m]), ep["raw"][m]
                side = "behind" if lead <= -a.margin else "ahead" if lead >= a.margin else None
                if side and raw:
                    rows[side].append((len(raw), max(raw.values())))
        out = {}
        for side, v in rows.items():
            kids, top = np.array([x[0] for x in v]), np.array([x[1] for x in v])
            out[side] = {"moves": len(v)}
            if len(v):
                out[side].update(distinct_root_children_median=float(np.median(kids)),
                                 distinct_root_children_p90=float(np.percentile(kids, 90)),
                                 largest_count_median=float(np.median(top)))
        res["rules"][name] = out
        print(name, json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
