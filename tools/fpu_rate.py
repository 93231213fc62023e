"""Diagnostic (GPU box): what first-play urgency costs in complete self-play games per second, and
what it does to the search.

The same net, the same arena size and the same seeds on both sides; "off" is the default engine, "on" has
fpu_reduction set (the root reduction defaults to it).  Each measurement is one fresh child process (an engine's
first batches pay for allocations and code loading): it plays `--warmup` untimed batches, then `--batches` timed
ones, the host wall time taken around SelfPlayEngine.run (which ends synchronised); the records are read after
the clock stops.  The variants alternate (on, off, on, off, ...) for `--rounds` rounds, so drift of the machine
hits both alike.  Nothing is asserted: the JSON holds every child's numbers, the spread of each variant over its
rounds, the ratio of the rates, the expansions per batch of both (the search goes deeper under the rule), the
mean distinct root children per move (info[5]) and the rule's two counters per searched move.  Whether a net
trained on these searches is stronger is not measured here.

    python tools/fpu_rate.py [--envs 4096] [--sims 100] [--r 0.25] [--root-r R] [--rounds 3] [--batches 6]
                             [--warmup 1] [--out FILE.json]
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
    kw = dict(fpu_reduction=a.r, fpu_root_reduction=a.root_r) if a.child == "on" else {}
    entries = a.sims * 9000 + 65536  # both variants alike (the automatic size depends on the free memory)
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, 15, net=net, max_moves=MOVES, arena_entries=entries, **kw)
    sec, unv, picks, exps, kids, edges, arena = [], [], [], [], [], [], []
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
            rec = eng.records()
            sec.append(dt)
            unv.append(st["fpu_unvisited_picks"])
            picks.append(st["fpu_picks"])
            exps.append(st["expansions"])
            edges.append(st["path_edges"])
            arena.append(st["max_arena"])
            kids.append(float(rec["info"][:, :MOVES, 5].mean()))
    eng.close()
    t = sum(sec)
    moves = a.envs * MOVES * len(sec)
    print(json.dumps({"variant": a.child, "s_per_batch": sec, "fpu_unvisited_picks": unv, "fpu_picks": picks,
                      "expansions": exps, "path_edges": edges, "max_arena": arena, "root_children_per_move": kids,
                      "games_per_s": a.envs * len(sec) / t, "fpu_unvisited_picks_per_move": sum(unv) / moves,
                      "fpu_picks_per_move": sum(picks) / moves, "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--r", type=float, default=0.25)
    ap.add_argument("--root-r", type=float, default=None, help="the reduction at depth 0 (default: --r)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=6, help="timed episode batches per child")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", choices=("on", "off"), default=None, help="(internal) play one variant and report")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.root_r is None:
        a.root_r = a.r
    if a.child:
        return child(a)
    runs = {"on": [], "off": []}
    fwd = ["--envs", a.envs, "--sims", a.sims, "--r", a.r, "--root-r", a.root_r, "--batches", a.batches,
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

    def per_batch(key):
        return {v: sum(sum(r[key]) for r in runs[v]) / (a.batches * a.rounds) for v in ("on", "off")}
    g_on, g_off = summary(runs["on"], "games_per_s"), summary(runs["off"], "games_per_s")
    exps = per_batch("expansions")
    res = {"config": {"envs": a.envs, "sims": a.sims, "fpu_reduction": a.r, "fpu_root_reduction": a.root_r,
                      "rounds": a.rounds, "batches": a.batches, "warmup": a.warmup, "hidden": a.hidden,
                      "nblocks": a.nblocks, "device": runs["off"][0]["device"],
                      "method": "host wall time around SelfPlayEngine.run (48 moves, ends synchronised); one fresh "
                                "child process per measurement, on and off alternating; seeds 1000 + batch; net "
                                "prior (torch.manual_seed(0) weights), no root noise"},
           "games_per_s": {"on": g_on, "off": g_off},
           "ratio_on_over_off": g_on["mean"] / g_off["mean"],
           "difference_exceeds_off_spread": abs(g_on["mean"] - g_off["mean"]) > g_off["spread"],
           "expansions_per_batch": exps,
           "expansions_ratio_on_over_off": exps["on"] / exps["off"],
           "path_edges_per_batch": per_batch("path_edges"),
           "max_arena_entries": {v: max(max(r["max_arena"]) for r in runs[v]) for v in ("on", "off")},
           "root_children_per_move": {v: sum(sum(r["root_children_per_move"]) for r in runs[v]) / (a.batches * a.rounds)
                                      for v in ("on", "off")},
           "fpu_unvisited_picks_per_move": summary(runs["on"], "fpu_unvisited_picks_per_move")["mean"],
           "fpu_picks_per_move": summary(runs["on"], "fpu_picks_per_move")["mean"],
           "not_measured": "whether a net trained on these searches is stronger",
           "children": runs}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
