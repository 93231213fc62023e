"""Diagnostic (GPU box): what forced playouts and policy target pruning cost in complete self-play
games per second, and how often they act.

The same net, the same arena size, the same seeds and the same root noise on both sides; "off" is the default
engine, "on" has forced_playouts_k set (and the pruning on).  Each measurement is one fresh child process (an
engine's first batches pay for allocations and code loading): it plays `--warmup` untimed batches, then
`--batches` timed ones, the host wall time taken around SelfPlayEngine.run (which ends synchronised).  The
variants alternate (on, off, on, off, ...) for `--rounds` rounds, so drift of the machine hits both alike.
Nothing is asserted: the JSON holds every child's numbers, the spread of each variant over its rounds, the
ratio of the rates, and the mean forced root picks and pruned visits per searched move.  Whether the pruned
targets train a stronger net is not measured here.

    python tools/forced_playouts_rate.py [--envs 4096] [--sims 100] [--k 2] [--alpha 0.3] [--eps 0.25]
                                         [--rounds 3] [--batches 6] [--warmup 1] [--out FILE.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "nypc-yacht-auction_amd"))
MOVES = 48  # every real game


def child(a):
    import torch
    from yacht_amd.engine import SelfPlayEngine
    from yacht_amd.nnet import YachtNNet, YkNet
    torch.manual_seed(0)
    net = YkNet(YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict(), a.hidden, a.nblocks)
    kw = dict(forced_playouts_k=a.k) if a.child == "on" else {}
    entries = a.sims * 9000 + 65536  # both variants alike (the automatic size depends on the free memory)
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, 15, net=net, max_moves=MOVES, arena_entries=entries,
                         dirichlet_alpha=a.alpha, dirichlet_eps=a.eps, **kw)
    sec, picks, cut, exps = [], [], [], []
    for b in range(a.warmup + a.batches):
        seed = 1000 + b  # the same seeds in every child
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(seed, 0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = eng.stats()
        if st["errors"]:
            raise SystemExit(f"engine error flags {st['errors']}")
        if b >= a.warmup:
            sec.append(dt)
            picks.append(st["forced_picks"])
            cut.append(st["pruned_visits"])
            exps.append(st["expansions"])
    eng.close()
    t = sum(sec)
    moves = a.envs * MOVES * len(sec)
    print(json.dumps({"variant": a.child, "s_per_batch": sec, "forced_picks": picks, "pruned_visits": cut,
                      "expansions": exps, "games_per_s": a.envs * len(sec) / t,
                      "forced_picks_per_move": sum(picks) / moves, "pruned_visits_per_move": sum(cut) / moves,
                      "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--k", type=float, default=2.0)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--eps", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=6, help="timed episode batches per child")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", choices=("on", "off"), default=None, help="(internal) play one variant and report")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {"on": [], "off": []}
    fwd = ["--envs", a.envs, "--sims", a.sims, "--k", a.k, "--alpha", a.alpha, "--eps", a.eps, "--batches", a.batches,
           "--warmup", a.warmup, "--hidden", a.hidden, "--nblocks", a.nblocks]
    for _ in range(a.rounds):
        for variant in ("on", "off"):  # a fresh process each: this one never opens the GPU
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant] + [str(x) for x in fwd],
                               capture_output=True, text=True, timeout=a.child_timeout)
            if p.returncode != 0:  # nothing more is started on the GPU after a failed child
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"child {variant} failed with status {p.returncode}")
            runs[variant].append(json.loads(p.stdout.strip().splitlines()[-1]))

    def summary(rs, key):
        v = [r[key] for r in rs]
        return {"runs": v, "mean": sum(v) / len(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    g_on, g_off = summary(runs["on"], "games_per_s"), summary(runs["off"], "games_per_s")
    res = {"config": {"envs": a.envs, "sims": a.sims, "k": a.k, "prune": True, "dirichlet_alpha": a.alpha,
                      "dirichlet_eps": a.eps, "rounds": a.rounds, "batches": a.batches, "warmup": a.warmup,
                      "hidden": a.hidden, "nblocks": a.nblocks, "device": runs["off"][0]["device"],
                      "method": "host wall time around SelfPlayEngine.run (48 moves, ends synchronised); one fresh "
                                "child process per measurement, on and off alternating; seeds 1000 + batch; root "
                                "noise on in both"},
           "games_per_s": {"on": g_on, "off": g_off},
           "ratio_on_over_off": g_on["mean"] / g_off["mean"],
           "difference_exceeds_off_spread": abs(g_on["mean"] - g_off["mean"]) > g_off["spread"],
           "forced_picks_per_move": summary(runs["on"], "forced_picks_per_move")["mean"],
           "pruned_visits_per_move": summary(runs["on"], "pruned_visits_per_move")["mean"],
           "expansions_per_batch": {v: sum(sum(r["expansions"]) for r in runs[v]) / (a.batches * a.rounds)
                                    for v in ("on", "off")},
           "not_measured": "whether the pruned targets train a stronger net",
           "children": runs}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
