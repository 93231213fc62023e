"""Diagnostic (GPU box): what the score-margin utility costs in complete self-play games per second,
how many descents it touches, and what the value-target call costs with it.

The same net, the same arena size and the same seeds on both sides; "off" is the default engine, "on" has
score_utility / score_scale set.  Each measurement is one fresh child process (an engine's first batches pay for
allocations and code loading): it plays `--warmup` untimed batches, then `--batches` timed ones, the host wall time
taken around SelfPlayEngine.run (which ends synchronised); the counters are read after the clock stops.  The
variants alternate (on, off, on, off, ...) for `--rounds` rounds, so drift of the machine hits both alike.  Every
child then times the value-target call over its last batch's packed image - yk_examples_value_targets in the
"off" child, yk_examples_utility_targets in the "on" child, both at (beta, lambda) = (--beta, --lam) on engines
that record root values - with HIP events around 10 back-to-back calls.  Nothing is asserted: the JSON holds every
child's numbers, the spread of each variant over its rounds, the ratio of the rates and the share of descents that
ended at a terminal state.  Whether a net trained on these targets is stronger is not measured here.

    python tools/score_utility_rate.py [--envs 4096] [--sims 100] [--weight 0.5] [--scale 20000] [--rounds 3]
                                       [--batches 4] [--warmup 1] [--out FILE.json]
"""
import argparse
import ctypes as C
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
    from yacht_amd._lib import call
    from yacht_amd.engine import SelfPlayEngine
    from yacht_amd.nnet import YachtNNet, YkNet
    torch.manual_seed(0)
    net = YkNet(YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict(), a.hidden, a.nblocks)
    on = a.child == "on"
    kw = dict(score_utility=a.weight, score_scale=a.scale) if on else {}
    entries = a.sims * 9000 + 65536  # both variants alike (the automatic size depends on the free memory)
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, 15, net=net, max_moves=MOVES, arena_entries=entries,
                         record_root_values=True, **kw)
    sec, terms, descents, exps = [], [], [], []
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
            terms.append(st["utility_terminals"])
            descents.append(a.envs * st["sims"])  # every game descends once per lock-step simulation
            exps.append(st["expansions"])
    img = eng.pack_records().reshape(1, -1)
    eng.close()
    n = a.envs * MOVES
    vals = torch.empty(n, dtype=torch.float32, device="cuda")
    rootv = torch.empty(n, dtype=torch.float32, device="cuda")
    out = C.c_int64()

    def targets_pass():
        if on:
            call("yk_examples_utility_targets", img.data_ptr(), 1, a.envs, MOVES, a.sims, -1, 0, n, a.beta, a.lam, a.weight,
                 a.scale, vals.data_ptr(), rootv.data_ptr(), C.byref(out), None)
        else:
            call("yk_examples_value_targets", img.data_ptr(), 1, a.envs, MOVES, a.sims, -1, 0, n, a.beta, a.lam,
                 vals.data_ptr(), rootv.data_ptr(), C.byref(out), None)
    targets_pass()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        targets_pass()
    e1.record()
    e1.synchronize()
    print(json.dumps({"variant": a.child, "s_per_batch": sec, "utility_terminals": terms, "descents": descents,
                      "expansions": exps, "games_per_s": a.envs * len(sec) / sum(sec),
                      "terminal_share_of_descents": sum(terms) / sum(descents),
                      "targets_ms_per_call": e0.elapsed_time(e1) / 10, "examples": n,
                      "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--scale", type=float, default=20000.0)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--lam", type=float, default=0.9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4, help="timed episode batches per child")
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
    fwd = ["--envs", a.envs, "--sims", a.sims, "--weight", a.weight, "--scale", a.scale, "--beta", a.beta, "--lam", a.lam,
           "--batches", a.batches, "--warmup", a.warmup, "--hidden", a.hidden, "--nblocks", a.nblocks]
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
    t_on, t_off = summary(runs["on"], "targets_ms_per_call"), summary(runs["off"], "targets_ms_per_call")
    res = {"config": {"envs": a.envs, "sims": a.sims, "score_utility": a.weight, "score_scale": a.scale, "beta": a.beta,
                      "lambda": a.lam, "rounds": a.rounds, "batches": a.batches, "warmup": a.warmup, "hidden": a.hidden,
                      "nblocks": a.nblocks, "device": runs["off"][0]["device"],
                      "method": "host wall time around SelfPlayEngine.run (48 moves, ends synchronised); one fresh "
                                "child process per measurement, on and off alternating; seeds 1000 + batch; net "
                                "prior (torch.manual_seed(0) weights), root values recorded on both sides; the "
                                "value-target call: HIP events around 10 calls over the child's last image"},
           "games_per_s": {"on": g_on, "off": g_off},
           "ratio_on_over_off": g_on["mean"] / g_off["mean"],
           "difference_exceeds_off_spread": abs(g_on["mean"] - g_off["mean"]) > g_off["spread"],
           "terminal_share_of_descents": summary(runs["on"], "terminal_share_of_descents")["mean"],
           "utility_terminals_per_batch": sum(sum(r["utility_terminals"]) for r in runs["on"]) / (a.batches * a.rounds),
           "expansions_per_batch": {v: sum(sum(r["expansions"]) for r in runs[v]) / (a.batches * a.rounds)
                                    for v in ("on", "off")},
           "targets_ms_per_call": {"on": t_on, "off": t_off, "examples": runs["on"][0]["examples"]},
           "not_measured": "whether a net trained on these targets is stronger; a sensible scale for a trained net",
           "children": runs}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
