"""Diagnostic (GPU box): what the self-play temperatures cost in complete self-play games per second.

Engines on the same net, the same arena size and the same seeds - everything off; the move schedule on; the root
schedule on; the root noise on; the root schedule and the noise on (one launch pair does both) - play whole
episode batches in turns (off, move, root, noise, root+noise, off, ...), each batch timed on the host around
SelfPlayEngine.run (which ends synchronised).  Every engine runs with the same tempThreshold (default 49: a draw
at every move, so the tempered draw is paid 48 times a game, not 14).  The median batch time of each, the games
per second and the ratios are reported - move / off, root / off, (root + noise) / noise - with the spread of the
off engine's own rounds to read them against, the expansions per batch (other searches are other work) and the
mean distinct visited root children per move (info[5]).  Nothing is asserted, and whether a net trained on these
games is stronger is not measured here.

    python tools/time_temper.py [--envs 4096] [--sims 100] [--rounds 5] [--warmup 1] [--temp-threshold 49]
                                [--move 0.75 0.15] [--root 1.25 1.1] [--halflife 16] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "nypc-yacht-auction_amd"))
from yacht_amd.engine import SelfPlayEngine  # noqa: E402
from yacht_amd.nnet import YachtNNet, YkNet  # noqa: E402

MOVES = 48  # every real game


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5, help="timed episode batches per variant")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--temp-threshold", type=int, default=49)
    ap.add_argument("--move", type=float, nargs=2, default=(0.75, 0.15), metavar=("EARLY", "FINAL"))
    ap.add_argument("--root", type=float, nargs=2, default=(1.25, 1.1), metavar=("EARLY", "FINAL"))
    ap.add_argument("--halflife", type=float, default=16.0)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--eps", type=float, default=0.25)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    net = YkNet(YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict(), a.hidden, a.nblocks)
    entries = a.sims * 9000 + 65536  # every engine alike (the automatic size depends on the free memory)
    move = dict(move_temperature=a.move[1], move_temperature_early=a.move[0], temperature_halflife=a.halflife)
    root = dict(root_policy_temperature=a.root[1], root_policy_temperature_early=a.root[0],
                temperature_halflife=a.halflife)
    noise = dict(dirichlet_alpha=a.alpha, dirichlet_eps=a.eps)
    variants = (("off", {}), ("move", move), ("root", root), ("noise", noise), ("root_noise", dict(root, **noise)))
    eng = {name: SelfPlayEngine(a.envs, a.sims, 1.5, a.temp_threshold, net=net, max_moves=MOVES,
                                arena_entries=entries, **kw) for name, kw in variants}
    sec = {name: [] for name in eng}
    exps = {name: [] for name in eng}
    kids = {}
    for r in range(a.warmup + a.rounds):
        for name, e in eng.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.run(1000 + r, 0)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = e.stats()
            if st["errors"]:
                raise SystemExit(f"engine error flags {st['errors']} ({name})")
            if r >= a.warmup:
                sec[name].append(dt)
                exps[name].append(st["expansions"])
    for name, e in eng.items():  # (after the clock: the last batch's records)
        kids[name] = float(e.records()["info"][:, :MOVES, 5].mean())
        e.close()
    med = {name: statistics.median(x) for name, x in sec.items()}
    res = {"config": {"envs": a.envs, "sims": a.sims, "rounds": a.rounds, "warmup": a.warmup,
                      "temp_threshold": a.temp_threshold, "move": list(a.move), "root": list(a.root),
                      "halflife": a.halflife, "alpha": a.alpha, "eps": a.eps, "hidden": a.hidden,
                      "nblocks": a.nblocks, "arena_entries": entries,
                      "method": "host wall time around SelfPlayEngine.run (48 moves, ends synchronised), the engines "
                                "taking turns batch by batch; median of the rounds",
                      "device": torch.cuda.get_device_name(0)},
           "variants": {name: {"s_per_batch_median": med[name], "s_per_batch_rounds": sec[name],
                               "games_per_s": a.envs / med[name], "expansions_per_batch": exps[name],
                               "distinct_root_children_per_move": kids[name]} for name in eng},
           "off_spread_percent": 100.0 * (max(sec["off"]) - min(sec["off"])) / med["off"],
           "games_per_s_ratio": {"move_over_off": med["off"] / med["move"], "root_over_off": med["off"] / med["root"],
                                 "noise_over_off": med["off"] / med["noise"],
                                 "root_noise_over_noise": med["noise"] / med["root_noise"]},
           "note": "a variant that searches other trees does other work: read the ratios beside the expansions per "
                   "batch; training strength is not measured"}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
