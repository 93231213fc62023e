"""Diagnostic (GPU box): what the Dirichlet root noise (dirichlet_alpha / dirichlet_eps) costs a
self-play batch.  Two engines on the same net and the same arena size, noise off and on, play whole episode
batches in turns (off, on, off, on, ...), each batch timed on the host around SelfPlayEngine.run (which ends
synchronised); the median batch time of each and their ratio are reported.  The sampler alone is timed too:
yk_dirichlet_noise on one row per game at the two root sizes of real play (202 bids, 3024 score actions), HIP
events around back-to-back launches - the same device function k_root_noise runs twice per move.

    python tools/time_root_noise.py [--envs 4096] [--sims 100] [--rounds 5] [--warmup 1] [--out FILE.json]
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
from yacht_amd import kernels as K  # noqa: E402
from yacht_amd.engine import SelfPlayEngine  # noqa: E402
from yacht_amd.nnet import YachtNNet, YkNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5, help="timed episode batches per variant")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--eps", type=float, default=0.25)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    net = YkNet(YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict(), a.hidden, a.nblocks)
    entries = a.sims * 9000 + 65536  # both engines alike (the automatic size depends on the free memory)
    eng = {name: SelfPlayEngine(a.envs, a.sims, 1.5, 15, net=net, max_moves=48, arena_entries=entries, **kw)
           for name, kw in (("off", {}), ("on", dict(dirichlet_alpha=a.alpha, dirichlet_eps=a.eps)))}
    sec = {name: [] for name in eng}
    exps = {}
    for r in range(a.warmup + a.rounds):
        for name, e in eng.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.run(r, 0)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = e.stats()
            if st["errors"]:
                raise SystemExit(f"engine error flags {st['errors']} ({name})")
            if r >= a.warmup:
                sec[name].append(dt)
                exps[name] = st["expansions"]
    for e in eng.values():
        e.close()
    # the sampler alone, one row per game
    sampler = {}
    env = torch.arange(a.envs, dtype=torch.int32, device="cuda")
    mv = torch.zeros(a.envs, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for V in (202, 3024):
        nv = torch.full((a.envs,), V, dtype=torch.int32, device="cuda")
        K.dirichlet_noise(1, env, mv, nv, a.alpha)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            K.dirichlet_noise(1, env, mv, nv, a.alpha)
        e1.record()
        e1.synchronize()
        sampler[f"V{V}_ms_per_launch"] = e0.elapsed_time(e1) / 10
    med = {name: statistics.median(x) for name, x in sec.items()}
    res = {"config": {"envs": a.envs, "sims": a.sims, "rounds": a.rounds, "warmup": a.warmup, "alpha": a.alpha,
                      "eps": a.eps, "hidden": a.hidden, "nblocks": a.nblocks, "arena_entries": entries,
                      "method": "host wall time around SelfPlayEngine.run (48 moves, ends synchronised), the two "
                                "engines taking turns batch by batch; median of the rounds",
                      "device": torch.cuda.get_device_name(0)},
           "off_s_per_batch": {"median": med["off"], "rounds": sec["off"]},
           "on_s_per_batch": {"median": med["on"], "rounds": sec["on"]},
           "expansions_per_batch": exps,
           "noise_overhead_percent": 100.0 * (med["on"] / med["off"] - 1.0),
           "sampler_alone": dict(sampler, rows=a.envs,
                                 note="yk_dirichlet_noise (the allocation of its output included), one row per game; "
                                      "k_root_noise runs the same device function once per game and move")}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
