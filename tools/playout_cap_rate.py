"""Diagnostic (GPU box): complete self-play games per second with the playout cap on and off.

The same net, the same arena size and the same seeds on both sides; "off" is the default engine, "on" has
playout_fast_sims / playout_full_prob set.  Each measurement is one fresh child process (an engine's first
batches pay for allocations and code loading, and a process that played the other variant has a warm cache):
it plays `--warmup` untimed batches, then `--batches` timed ones, the host wall time taken around
SelfPlayEngine.run (which ends synchronised).  The variants alternate (on, off, on, off, ...) for `--rounds`
rounds, so drift of the machine hits both alike.  Nothing is asserted: the JSON holds every child's numbers,
the spread of each variant over its rounds, and whether the capped rate exceeds the uncapped one by more than
the uncapped runs' own spread.

    python tools/playout_cap_rate.py [--envs 4096] [--sims 100] [--fast-sims 20] [--full-prob 0.25]
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
    kw = dict(playout_fast_sims=a.fast_sims, playout_full_prob=a.full_prob) if a.child == "on" else {}
    entries = a.sims * 9000 + 65536  # both variants alike (the automatic size depends on the free memory)
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, 15, net=net, max_moves=MOVES, arena_entries=entries, **kw)
    sec, sims_run, full, exps = [], [], [], []
    for b in range(a.warmup + a.batches):
        seed = 1000 + b  # the same seeds in every child: the same schedules in every "on" child
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
            sims_run.append(st["sims"])
            full.append(MOVES - st["fast_moves"])
            exps.append(st["expansions"])
    eng.close()
    t = sum(sec)
    print(json.dumps({"variant": a.child, "s_per_batch": sec, "lockstep_sims": sims_run, "full_moves": full,
                      "expansions": exps, "games_per_s": a.envs * len(sec) / t,
                      "full_examples_per_s": a.envs * sum(full) / t, "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--fast-sims", type=int, default=20)
    ap.add_argument("--full-prob", type=float, default=0.25)
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
    fwd = ["--envs", a.envs, "--sims", a.sims, "--fast-sims", a.fast_sims, "--full-prob", a.full_prob, "--batches",
           a.batches, "--warmup", a.warmup, "--hidden", a.hidden, "--nblocks", a.nblocks]
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
    sims_on = sum(sum(r["lockstep_sims"]) for r in runs["on"])
    sims_off = sum(sum(r["lockstep_sims"]) for r in runs["off"])
    res = {"config": {"envs": a.envs, "sims": a.sims, "fast_sims": a.fast_sims, "full_prob": a.full_prob,
                      "rounds": a.rounds, "batches": a.batches, "warmup": a.warmup, "hidden": a.hidden,
                      "nblocks": a.nblocks, "device": runs["off"][0]["device"],
                      "method": "host wall time around SelfPlayEngine.run (48 moves, ends synchronised); one fresh "
                                "child process per measurement, on and off alternating; seeds 1000 + batch"},
           "games_per_s": {"on": g_on, "off": g_off},
           "full_examples_per_s": {"on": summary(runs["on"], "full_examples_per_s"),
                                   "off": summary(runs["off"], "full_examples_per_s")},
           "speedup_games": g_on["mean"] / g_off["mean"],
           "speedup_bound_expected": a.sims / (a.full_prob * a.sims + (1.0 - a.full_prob) * a.fast_sims),
           "speedup_bound_these_seeds": sims_off / sims_on,  # the lock-step simulations actually saved
           "on_exceeds_off_by_more_than_off_spread": g_on["mean"] - g_off["mean"] > g_off["spread"],
           "children": runs}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
