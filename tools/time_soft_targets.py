"""Diagnostic (GPU box): what the soft-target train step (policy_target="visits") costs over the
hard-target one.  A self-play shard (its visit-policy CSR is what the soft step trains on), then
the native step at one batch size in four variants - f32 / amp x hard / soft - each timed with HIP
events around runs of back-to-back steps after a warm-up, the median over the rounds reported.
The variants take turns round by round, so clock or thermal drift lands on all four alike.

    python tools/time_soft_targets.py [--batch 512] [--steps 50] [--rounds 15] [--warmup 20] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "nypc-yacht-auction_amd"))
from yacht_amd.engine import SelfPlayEngine  # noqa: E402
from yacht_amd.nnet import YachtNNet, YkNet  # noqa: E402
from yacht_amd.replay import as_device_policies, examples_from_images  # noqa: E402
from yacht_amd.train import Trainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50, help="back-to-back steps per timed run")
    ap.add_argument("--rounds", type=int, default=15, help="timed runs per variant")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=256, help="self-play games behind the shard")
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--temp-threshold", type=int, default=48, help="moves played at temperature 1 (visit policies)")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--nblocks", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    sd = YachtNNet(hidden=a.hidden, nblocks=a.nblocks).state_dict()
    eng = SelfPlayEngine(a.envs, a.sims, 1.5, a.temp_threshold, net=YkNet(sd, a.hidden, a.nblocks), max_moves=48)
    eng.run(0, 0)
    shard = examples_from_images(eng.pack_records(), a.envs, 48, a.sims)
    eng.close()
    S, T, V, pol = shard.states, shard.targets, shard.values, as_device_policies(shard)
    n = len(shard)
    nnz = int(pol[0][-1]) / n
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    perm = torch.randperm(n, generator=g, device="cuda").to(torch.int32)
    idx = [perm[j:j + a.batch].contiguous() for j in range(0, n - a.batch + 1, a.batch)]
    variants = [(amp, soft) for amp in (False, True) for soft in (False, True)]
    tr = {v: Trainer(sd, a.hidden, a.nblocks, max_batch=a.batch, dropout=0.3, amp=v[0]) for v in variants}
    step = lambda v, i: tr[v].step(S, T, V, idx=idx[i % len(idx)], policies=pol if v[1] else None)
    for v in variants:
        for i in range(a.warmup):
            step(v, i)
    ms = {v: [] for v in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(a.rounds):
        for v in variants:
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.steps):
                step(v, r * a.steps + i)
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1) / a.steps)
    res = {"config": {"batch": a.batch, "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup, "hidden": a.hidden,
                      "nblocks": a.nblocks, "examples": n, "mean_nnz_per_policy": nnz, "dropout": 0.3,
                      "shard": f"{a.envs} self-play games x {a.sims} sims, {a.temp_threshold} moves at temperature 1",
                      "method": "HIP events around runs of `steps` back-to-back steps, the four variants taking "
                                "turns round by round; median (p10, p90) of the rounds' time per step",
                      "device": torch.cuda.get_device_name(0)}}
    for amp, soft in variants:
        x = sorted(ms[(amp, soft)])
        res[("amp" if amp else "f32") + "_" + ("soft" if soft else "hard") + "_ms_per_step"] = {
            "median": statistics.median(x), "p10": x[len(x) // 10], "p90": x[(9 * len(x)) // 10], "rounds": x}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
